"""SMAP inference entry point on MI355X (reference: exps/stage3_root2/test.py).

Same command line (test.py:156-177) and the same result JSON
(`<exp>_<mode>_<data_mode>_<suffix>.json` with `model_pattern` and `3d_pairs`, test.py:32-38,147-151):

    export PROJECT_HOME=/path/to/repo ; export PYTHONPATH=$PYTHONPATH:$PROJECT_HOME
    python test.py -p SMAP_model.pth -t run_inference -d test [-rp RefineNet.pth] \
           --batch_size 16 --do_flip 1 --dataset_path /path/to/images

Per batch everything stays on the GPU: HIP backbone -> optional flip-TTA merge -> /255,/127 ->
batched association -> batched lifting (-> RefineNet); only the poses come back, and the
post-processing of batch k overlaps the backbone of batch k+1 (smap_amd/pipeline.py).  Launched under
`torch.distributed.run` the image list is split in contiguous per-rank blocks
(lib/utils/dataloader.py:80-85) and the records are gathered with one RCCL all_gather.

The ground-truth modes (test.py:73-95,142-143) run on the same pipeline: `-t generate_result` registers the
persons to the annotations of cfg.TEST.JSON_PATH on the device (smap_register_gt) and writes one record per frame
with the ground truth attached (the input of lib/eval/convert.py); `-t generate_train -d generation|test` writes
one record per matched person, the RefineNet training pairs (dataset/p2p_dataset.py).

`-t generate_result --eval_3d 1` (addition) scores the run while it runs: MPJPE, root-relative error, PCK, point / person recall
and the depth-order reverse rate of lib/eval/test_util_panoptic.py (eval_3d, calculate_and_log), accumulated on the GPU
(smap_amd/evaluate.py) and written as `error` into the result file, as the reference's Panoptic test does.

`-t generate_result --eval_maps 1` (addition), with or without --eval_3d, scores the network's MAPS: head-size-normalised 2D keypoint error,
keypoint recall and the per-bone relative-depth error / reverse count of that module's `eval` branch (eval_one_image, generate_rootZ),
accumulated on the GPU next to the lifting kernel (smap_amd/evaluate.py EvalMaps); the six raw accumulators are added to `error`.

`-t generate_result --eval_mupots ROOT` (addition) scores the finished run by the MuPoTS-3D protocol (lib/eval/mupots_smap.m: 3DPCK, AUC,
MPJPE, ordinal rate; smap_amd/mupots.py on the GPU) against TS<k>/annot.mat and TS<k>/occlusion.mat under ROOT and writes the summary
into error["mupots"] of the result file: lib/eval/convert.py and the MATLAB step in one.

`-t generate_result|generate_train --maps_from_gt 1` (addition): the maps of every batch are RENDERED from the frame's annotations on the
GPU (smap_amd/labels.py: what a perfectly trained backbone would return) instead of coming from the backbone: no checkpoint, no engine,
no image file; everything behind the maps is unchanged.  Checks an annotation file end to end and measures the ceiling of association +
lifting on it.

`--device_preprocess 1 [--device_decode 1|2]` (addition) acts in all three modes: the frames are decoded ahead of the consumer and resized /
padded / normalised on the GPU, one launch per batch (smap_amd/loaders.py: DevicePreprocLoader); the result file is the same.

The script itself: parse_args (the flags and the table of combinations that are refused), make_loader (which dataset on which loader),
generate_3d_point_pairs (the run: shape_batch / pad_to per loader batch, the pipeline, gather, scorers, result file) and main."""
import argparse
import json
import logging
import os
import sys
import time
from typing import NamedTuple

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Subset

from model.smap import SMAP
from model.refinenet import RefineNet
from dataset.custom_dataset import CustomDataset
from smap_amd.dist import gather_records, init_single_rank_group, shard_range
from exps.stage3_root2.config import cfg
from smap_amd.loaders import AnnotationLoader, DevicePreprocLoader
from smap_amd.pipeline import DryRunPipeline, make_pipeline
from exps.stage3_root2.test_util import default_cams
from smap_amd.records import annotation_camera, kept_annotations, to_jsonable


def get_logger(name, log_dir, filename):
    os.makedirs(log_dir, exist_ok=True)
    logger = logging.getLogger(name)
    if not logger.handlers:
        logger.setLevel(logging.INFO)
        fmt = logging.Formatter("%(asctime)s %(levelname)s %(message)s")
        for h in (logging.StreamHandler(), logging.FileHandler(os.path.join(log_dir, filename))):
            h.setFormatter(fmt)
            logger.addHandler(h)
    return logger


def gathering():
    """The ranks' records and scores are gathered at the end of the run: a launch of several ranks, or one rank that asks for it (tests)."""
    return dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("SMAP_FORCE_GATHER", "") == "1")


class _NoFrames:
    """What the loop reads of a batch of frames (its length and shape) when there are none (--maps_from_gt 1)."""

    def __init__(self, n, input_shape):
        self.shape = (n, 3, int(input_shape[0]), int(input_shape[1]))

    def __len__(self):
        return self.shape[0]


class Batch(NamedTuple):
    """What the pipeline's submit takes of one loader batch; every member but map_inputs (a pair of such) has one entry per frame."""
    imgs: object               # [n,3,H,W] fp32 on the device, or _NoFrames: no frames, this shape
    cams: object               # n rows of 9
    tags: list                 # the frames' names in the records; None = a padding frame, no record
    annotations: object        # ground-truth modes: the kept annotations [G_i,15,C] of every frame
    map_inputs: object         # --maps_from_gt 1: (annotations as loaded, scales) the maps are rendered from


def shape_batch(batch, cfg, device, maps_from_gt=False):
    """A loader batch -- (imgs, names, scales) of an image folder, (imgs or None, annotations, names, scales) of an annotated set -- as a Batch."""
    on_device = lambda imgs: imgs.to(device, non_blocking=True).float().contiguous()
    if cfg.TEST_MODE == "run_inference":
        imgs, names, scales = batch
        return Batch(on_device(imgs), default_cams(scales, len(imgs)), list(names), None, None)
    imgs, meta_data, names, scales = batch                       # test.py:50-51,73-95
    annotations = [kept_annotations(m.numpy(), cfg.DATASET.ROOT_IDX) for m in meta_data]
    cams = [annotation_camera(a, s) if len(a) else [1.0] * 9 for a, s in zip(annotations, scales)]
    if maps_from_gt:
        return Batch(_NoFrames(len(names), cfg.dataset.INPUT_SHAPE), cams, list(names), annotations, (list(meta_data), list(scales)))
    return Batch(on_device(imgs), cams, list(names), annotations, None)


def pad_to(b, B):
    """A ragged last batch as a batch of B: padded with copies of its last frame whose records are dropped (tag None) -- no second
    engine / arena.  A batch that is full already comes back as it is."""
    pad = B - len(b.tags)
    if pad <= 0:
        return b
    more = lambda seq: list(seq) + [seq[-1]] * pad
    cams = np.asarray(b.cams, np.float64)
    return Batch(_NoFrames(B, b.imgs.shape[2:]) if isinstance(b.imgs, _NoFrames) else torch.cat([b.imgs, b.imgs[-1:].expand(pad, -1, -1, -1)], 0).contiguous(),
                 np.concatenate([cams, np.repeat(cams[-1:], pad, 0)], 0), b.tags + [None] * pad,
                 None if b.annotations is None else more(b.annotations), None if b.map_inputs is None else tuple(more(m) for m in b.map_inputs))


def score_mupots(result, mupots_ann, device, logger):
    """error["mupots"] of `result` from its jsonable records, as the file will hold them.  -> the exception when the scorer refuses or
    fails: the caller writes the pairs all the same and raises it afterwards."""
    from lib.eval.convert import convert_records
    from smap_amd.mupots import MuPoTSScorer
    try:
        pose3d, pose2d, _ = convert_records(result["3d_pairs"])
        summary = MuPoTSScorer(mupots_ann, device=device).score(pose2d, pose3d).summary()
        logger.info("MuPoTS-3D: 3DPCK {mean_pck:.4g}  AUC {mean_auc:.4g}  MPJPE {mean_mpjpe:.6g} mm (means over the sequences)".format(**summary))
        result.setdefault("error", {})["mupots"] = summary
    except Exception as exc:
        return exc


def generate_3d_point_pairs(model, refine_model, data_loader, cfg, logger, device, output_dir="", pipeline_cls=None, eval_3d=False, eval_maps=False,
                            maps_from_gt=False, eval_loss=False, eval_mupots=None):
    os.makedirs(output_dir, exist_ok=True)
    mupots_ann = None
    if eval_mupots:                # read before the run: a wrong root is refused at once
        from smap_amd.mupots import load_annotations
        mupots_ann = load_annotations(eval_mupots)
    source = {}
    if maps_from_gt:               # the batches carry no frames (AnnotationLoader): their maps are rendered from the annotations
        from smap_amd.labels import GtMapsSource, label_spec
        source["maps_source"] = GtMapsSource(label_spec(cfg), device)
    if pipeline_cls is None:       # batches of <= 8 frames share a backbone launch (smap_amd/pipeline.py::make_pipeline, SMAP_LAUNCH_FRAMES)
        pipeline_cls = lambda m, c, b, h, w, d, rw, **kw: make_pipeline(m, c, b, h, w, d, refine_weights=rw, **kw)
    evaluators = {}                # pipeline argument -> evaluator, 3D first: the order of the log lines and of result["error"]
    if eval_3d:                    # the reference's `error` dict, accumulated on the device by every batch's post-processing
        from smap_amd.evaluate import Eval3D
        evaluators["evaluator"] = Eval3D(device, refine=refine_model is not None)
    if eval_maps:                  # the `eval` keys of that dict: 2D keypoint error / recall and bone depth error of the maps
        from smap_amd.evaluate import EvalMaps
        evaluators["map_evaluator"] = EvalMaps(device)
    if model is not None:
        model.eval()
    val_loss = None
    if eval_loss:                  # the validation loss: SMAP.forward(imgs, valids, labels, rdepth) on every batch's own frames
        from smap_amd.loss import ValidationLoss
        val_loss = ValidationLoss(model, cfg, device)
    scorers = list(evaluators.values()) + ([val_loss] if val_loss is not None else [])     # in the order of their keys in result["error"]
    refine_w = None
    if refine_model is not None:
        refine_model.eval()
        refine_w = refine_model.folded(device)
    result = dict()
    result["model_pattern"] = cfg.DATASET.NAME
    result["3d_pairs"] = []
    rank = dist.get_rank() if dist.is_initialized() else 0
    it = data_loader
    if rank == 0:
        try:
            from tqdm import tqdm
            it = tqdm(data_loader)
        except ImportError:
            pass
    pipe = None
    dropped = []                     # frames without a result: their maps came out non-finite

    def drain(recs):
        if recs:
            result["3d_pairs"].extend(recs)

    def retire(p):                   # a pipeline that is replaced or finished: everything in flight + the frames it dropped
        drain(p.flush())
        dropped.extend(getattr(p, "dropped_frames", []))

    clock = {"loader_s": 0.0, "submit_s": 0.0, "frames": 0, "t0": time.perf_counter()}     # where the host's time goes (SMAP_CLI_TIMING)
    batches = iter(it)
    while True:
        t_ = time.perf_counter()
        try:
            batch = next(batches)
        except StopIteration:
            break
        clock["loader_s"] += time.perf_counter() - t_
        t_sub = time.perf_counter()
        b = shape_batch(batch, cfg, device, maps_from_gt)
        if val_loss is not None:                                 # before the padding: the batch's real frames, unmirrored, a forward of its own
            val_loss.update(b.imgs, batch[1], batch[3])
        if pipe is not None:
            b = pad_to(b, pipe.B)
        if pipe is None or pipe.B != len(b.imgs):                # a change of batch size: a new pipeline
            if pipe is not None:
                retire(pipe)
            pipe = pipeline_cls(model, cfg, len(b.imgs), b.imgs.shape[-2], b.imgs.shape[-1], device, refine_w,
                                do_flip=bool(cfg.DO_FLIP), record_mode=cfg.TEST_MODE, numpy_records=True,
                                depth=int(os.environ.get("SMAP_PIPELINE_DEPTH", 2)),   # two backbones in flight (+19 %)
                                **evaluators, **source)
        with torch.no_grad():
            if maps_from_gt:
                drain(pipe.submit(None, b.cams, list(b.tags), annotations=b.annotations, map_inputs=b.map_inputs))
            else:
                drain(pipe.submit(b.imgs, b.cams, list(b.tags), annotations=b.annotations))
        clock["submit_s"] += time.perf_counter() - t_sub
        if "first_submit_s" not in clock:                        # builds the engine (schedule, weight packing, plan, arenas): seconds, once
            clock["first_submit_s"] = time.perf_counter() - t_sub
        clock["frames"] += sum(1 for t in b.tags if t is not None)
    t_ = time.perf_counter()
    if pipe is not None:
        retire(pipe)
    clock["flush_s"] = time.perf_counter() - t_
    clock["loop_s"] = time.perf_counter() - clock.pop("t0")
    if os.environ.get("SMAP_CLI_TIMING") and rank == 0:
        # steady-state split of the run_inference loop: loader_s = waiting for the next batch (decode [+ host resize] + H2D + GPU
        # pre-processing enqueue), submit_s = enqueue + back-pressure of the pipeline + record building, flush_s = draining the tail
        steady = clock["loop_s"] - clock.get("first_submit_s", 0.0)
        clock.update(frames_per_s=clock["frames"] / clock["loop_s"] if clock["loop_s"] > 0 else None,
                     frames_per_s_after_engine_build=clock["frames"] / steady if steady > 0 else None, wait_gpu_s=getattr(pipe, "wait_s", None))
        with open(os.environ["SMAP_CLI_TIMING"], "w") as f:
            json.dump(clock, f)
    if gathering():
        parts = gather_records(result["3d_pairs"], device)
        result["3d_pairs"] = [r for part in parts for r in part]                # rank order == frame order
        dropped = [n for part in gather_records(dropped, device) for n in part]
    if dropped:
        # the reference's fp32 forward has no such failure: say so where the caller will look (the result file and the exit status)
        result["dropped_frames"] = list(dropped)
        logger.warning("{} frame(s) have no result (non-finite maps: an activation exceeded the fp16 range, INTEGRATION.md section 5): {}".format(
            len(dropped), dropped[:20]))
    for scorer in scorers:
        raw = scorer.raw()                                                      # the run's only read-back of the scores
        if gathering():
            raw = scorer.merge_raws(gather_records(raw, device))                # rank order; evaluate.merge / merge_maps say what that costs
        if rank == 0:
            for line in scorer.log_lines(raw):                                  # calculate_and_log's lines (test_util_panoptic.py:388-400, :374-378)
                logger.info(line)
            result.setdefault("error", {}).update(scorer.result_entry(raw))
    if rank == 0:
        dir_name = os.path.split(os.path.split(os.path.realpath(__file__))[0])[1]
        name = os.path.join(output_dir, "{}_{}_{}_{}.json".format(dir_name, cfg.TEST_MODE, cfg.DATA_MODE,
                                                                  cfg.JSON_SUFFIX_NAME))
        result["3d_pairs"] = to_jsonable(result["3d_pairs"])          # ndarray -> nested lists, once, at the end of the run
        mupots_refusal = score_mupots(result, mupots_ann, device, logger) if mupots_ann is not None else None
        with open(name, "w") as f:
            json.dump(result, f)
        logger.info("Pairs writed to {}".format(name))
        if mupots_refusal is not None:                                # refused or failed: the pairs are written all the same
            raise mupots_refusal
    return result


_NO_RESULT = lambda a: a.test_mode != "generate_result"
# Combinations of flags that are refused: (applies to args, message -- str.format on the flags' values).  Checked in this order: the first wins.
FLAG_RULES = (
    (lambda a: a.eval_mupots and _NO_RESULT(a), "--eval_mupots requires -t generate_result"),
    (lambda a: a.eval_mupots and a.dry_run, "--eval_mupots scores on the GPU: not available with --dry_run 1"),
    (lambda a: a.eval_loss and _NO_RESULT(a), "--eval_loss 1 requires -t generate_result"),
    (lambda a: a.eval_loss and a.dry_run, "--eval_loss 1 runs on the GPU: not available with --dry_run 1"),
    (lambda a: a.eval_loss and a.maps_from_gt, "--eval_loss 1 needs the network's heads: not available with --maps_from_gt 1"),
    (lambda a: a.maps_from_gt and a.test_mode == "run_inference",
     "--maps_from_gt 1 renders the maps from annotations: -t run_inference has none (use -t generate_result or generate_train)"),
    (lambda a: a.maps_from_gt and a.dry_run, "--maps_from_gt 1 renders on the GPU: not available with --dry_run 1"),
    (lambda a: a.device_decode not in (0, 1, 2), "--device_decode is 0, 1 or 2"),
    (lambda a: a.device_decode and not a.device_preprocess, "--device_decode {device_decode} requires --device_preprocess 1"),
    (lambda a: a.eval_3d and _NO_RESULT(a), "--eval_3d 1 requires -t generate_result"),
    (lambda a: a.eval_3d and a.dry_run, "--eval_3d 1 scores on the GPU: not available with --dry_run 1"),
    (lambda a: a.eval_maps and _NO_RESULT(a), "--eval_maps 1 requires -t generate_result"),
    (lambda a: a.eval_maps and a.dry_run, "--eval_maps 1 scores on the GPU: not available with --dry_run 1"),
)


def parse_args(argv=None):
    """The command line (sys.argv[1:] when argv is None) -> args; a combination of FLAG_RULES is refused as argparse refuses (exit status 2)."""
    parser = argparse.ArgumentParser()
    parser.add_argument("--test_mode", "-t", type=str, default="run_inference",
                        choices=["generate_train", "generate_result", "run_inference"])
    parser.add_argument("--data_mode", "-d", type=str, default="test", choices=["test", "generation"])
    parser.add_argument("--SMAP_path", "-p", type=str, default="log/SMAP.pth", help="Path to SMAP model")
    parser.add_argument("--RefineNet_path", "-rp", type=str, default="",
                        help="Path to RefineNet model, empty means without RefineNet")
    parser.add_argument("--batch_size", type=int, default=1, help="Batch_size of test")
    parser.add_argument("--do_flip", type=float, default=0, help="Set to 1 if do flip when test")
    parser.add_argument("--dataset_path", type=str, default="", help='Image dir path of "run_inference" test mode')
    parser.add_argument("--json_name", type=str, default="", help="Add a suffix to the result json.")
    parser.add_argument("--precision", type=str, default="", choices=["", "x3", "f16"],
                        help="(addition) backbone arithmetic: x3 (default) = fp16 hi/lo pairs, three MFMAs per K step -- "
                             "reproduces the reference's fp32 forward; f16 = fp16 storage, ~2x faster, ~1e-3 relative error")
    parser.add_argument("--dry_run", type=int, default=0,
                        help="1: rehearse the run without a GPU or a checkpoint (stand-in pipeline, gloo gather): what a "
                             "multi-rank launch does around the device work -- split, ragged batches, gather, result file")
    parser.add_argument("--device_preprocess", type=int, default=0,
                        help="(addition) 1: resize/pad/normalise on the GPU (smap_preprocess_batch) instead of in the dataset, decodes ahead of "
                             "the consumer on a thread pool; in all three test modes")
    parser.add_argument("--device_decode", type=int, default=0,
                        help="(addition) 1: baseline JPEGs are Huffman-decoded on the host and finished on the GPU (smap_amd/jpeg.py), "
                             "bit for bit the PIL frame; other files are decoded with PIL.  2: the Huffman decode runs on the GPU too "
                             "(verified there; a frame it does not vouch for is redone on the host).  Requires --device_preprocess 1")
    parser.add_argument("--eval_3d", type=int, default=0, choices=[0, 1],
                        help="(addition) 1, with -t generate_result: score the run on the GPU (MPJPE, PCK, recall, reverse rate: "
                             "lib/eval/test_util_panoptic.py eval_3d) and write the `error` dict into the result file")
    parser.add_argument("--eval_maps", type=int, default=0, choices=[0, 1],
                        help="(addition) 1, with -t generate_result: score the network's maps on the GPU (2D keypoint error / recall, "
                             "bone depth error: lib/eval/test_util_panoptic.py eval_one_image, generate_rootZ) and add the six raw "
                             "accumulators to the `error` dict of the result file")
    parser.add_argument("--maps_from_gt", type=int, default=0, choices=[0, 1],
                        help="(addition) 1, with -t generate_result or generate_train: render the maps of every frame from its annotations "
                             "on the GPU (smap_amd/labels.py) instead of running the backbone: no checkpoint, no image file is read")
    parser.add_argument("--eval_loss", type=int, default=0, choices=[0, 1],
                        help="(addition) 1, with -t generate_result: the validation loss of the checkpoint (SMAP.forward with labels rendered "
                             "from every batch's annotations) as frame-weighted means into error['loss'] of the result file.  One more "
                             "forward per batch; the value depends on --batch_size, as the training log's does")
    parser.add_argument("--eval_mupots", metavar="ROOT", default="",
                        help="(addition) with -t generate_result: score the run by the MuPoTS-3D protocol on the GPU (3DPCK, AUC, MPJPE, "
                             "ordinal rate: lib/eval/mupots_smap.m) against TS<k>/annot.mat + occlusion.mat under ROOT and write the "
                             "summary into error['mupots'] of the result file")
    args = parser.parse_args(argv)
    for applies, message in FLAG_RULES:
        if applies(args):
            parser.error(message.format(**vars(args)))
    return args


def make_loader(args, cfg, logger, world, local, dry):
    """The run's batches: an image folder (-t run_inference), or the annotated set of cfg.TEST.JSON_PATH on the host loader
    (lib/utils/dataloader.py), on the device loader (--device_preprocess 1), or without its frames (--maps_from_gt 1).  Every rank
    takes its contiguous block."""
    rank = dist.get_rank() if world > 1 else 0
    if args.test_mode == "run_inference":
        dataset = CustomDataset(cfg, args.dataset_path)
        indices = range(*shard_range(len(dataset), world, rank)) if world > 1 else range(len(dataset))
    elif args.maps_from_gt or (args.device_preprocess and not dry):
        from dataset.base_dataset import JointDataset
        from lib.utils.dataloader import rank_block
        if cfg.DATASET.NAME != "MIX":                          # get_test_loader's check
            raise NameError("Dataset is not defined!", cfg.DATASET.NAME)
        dataset = JointDataset(cfg, args.data_mode)
        indices = range(*rank_block(len(dataset), world, rank))                # get_test_loader's split
        if args.maps_from_gt:
            if args.device_preprocess:
                logger.info("--maps_from_gt 1: no frame is read, --device_preprocess / --device_decode are ignored")
            return AnnotationLoader(dataset, indices, args.batch_size)
    else:
        from lib.utils.dataloader import get_test_loader
        if args.device_preprocess:
            logger.info("--dry_run 1: the ground-truth modes are rehearsed on the host loader (--device_preprocess needs the GPU)")
        return get_test_loader(cfg, num_gpu=world, local_rank=rank, stage=args.data_mode)
    if args.device_preprocess:
        return DevicePreprocLoader(dataset, indices, args.batch_size, cfg, torch.device(cfg.MODEL.DEVICE, local), device_decode=args.device_decode)
    return DataLoader(Subset(dataset, indices) if world > 1 else dataset, batch_size=args.batch_size, shuffle=False)


def main():
    # the schedule of a (checkpoint, shape, arithmetic) is built once and kept on disk (smap_amd/engine.py plan cache): the second start of
    # this command loads it through smap_plan_create_from_blob instead of re-packing the weights (SMAP_PLAN_CACHE=0 switches it off)
    os.environ.setdefault("SMAP_PLAN_CACHE", os.path.join(os.environ.get("XDG_CACHE_HOME", os.path.expanduser("~/.cache")), "smap_amd"))
    args = parse_args()
    cfg.TEST_MODE = args.test_mode
    cfg.DATA_MODE = args.data_mode
    cfg.REFINE = len(args.RefineNet_path) > 0
    cfg.DO_FLIP = args.do_flip
    cfg.JSON_SUFFIX_NAME = args.json_name
    cfg.TEST.IMG_PER_GPU = args.batch_size

    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    dry = bool(args.dry_run)
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("gloo" if dry else "nccl")
    elif world == 1 and os.environ.get("SMAP_FORCE_GATHER", "") == "1" and not dist.is_initialized():
        init_single_rank_group("gloo" if dry else "nccl")      # one rank, real collectives: the RCCL path on a one-GPU box (tests)
    if not dry:
        torch.cuda.set_device(local)
    os.makedirs(cfg.TEST_DIR, exist_ok=True)
    logger = get_logger(cfg.DATASET.NAME, cfg.TEST_DIR, "test_log_{}.txt".format(args.test_mode))

    device = torch.device("cpu") if dry else torch.device(cfg.MODEL.DEVICE, local)
    model = None
    if args.maps_from_gt:
        if args.do_flip or args.precision:
            logger.info("--maps_from_gt 1: no backbone runs, --do_flip and --precision are ignored")
        cfg.DO_FLIP = 0
    elif not dry:
        model = SMAP(cfg, run_efficient=cfg.RUN_EFFICIENT)
        model.to(device)
        if args.precision:
            model.precision = args.precision
    data_loader = make_loader(args, cfg, logger, world, local, dry)

    if dry:
        generate_3d_point_pairs(None, None, data_loader, cfg, logger, device, output_dir=os.path.join(cfg.OUTPUT_DIR, "result"),
                                pipeline_cls=DryRunPipeline)
        if dist.is_initialized():
            dist.destroy_process_group()
        return
    refine_model = RefineNet().to(device) if cfg.REFINE else None
    if args.maps_from_gt or os.path.exists(args.SMAP_path):
        if not args.maps_from_gt:
            state_dict = torch.load(args.SMAP_path, map_location=lambda storage, loc: storage)
            model.load_state_dict(state_dict["model"])
        if refine_model is not None:
            if os.path.exists(args.RefineNet_path):
                refine_model.load_state_dict(torch.load(args.RefineNet_path, map_location="cpu"))
            else:
                logger.info("No such RefineNet checkpoint of {}".format(args.RefineNet_path))
                return
        result = generate_3d_point_pairs(model, refine_model, data_loader, cfg, logger, device,
                                         output_dir=os.path.join(cfg.OUTPUT_DIR, "result"), eval_3d=bool(args.eval_3d),
                                         eval_maps=bool(args.eval_maps), maps_from_gt=bool(args.maps_from_gt), eval_loss=bool(args.eval_loss),
                                         eval_mupots=args.eval_mupots or None)
        if dist.is_initialized():
            dist.destroy_process_group()
        if result.get("dropped_frames"):
            return 2                 # the result file is written, but it lacks frames the reference would have produced
    else:
        logger.info("No such checkpoint of SMAP {}".format(args.SMAP_path))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
