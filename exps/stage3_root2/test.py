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
padded / normalised on the GPU, one launch per batch (DevicePreprocLoader below); the result file is the same."""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Subset

from model.smap import SMAP
from model.refinenet import RefineNet
from dataset.custom_dataset import CustomDataset
from smap_amd.dist import gather_records, shard_range
from exps.stage3_root2.config import cfg
from smap_amd.pipeline import PosePipeline, make_pipeline
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


class DevicePreprocLoader:
    """Batches of (imgs on the device, names, scales) with decode on the host and resize / pad /
    normalise in one HIP launch per batch of up to 16 frames (smap_amd/preprocess.py: smap_preprocess_batch).  The decodes run AHEAD of the consumer on a small thread pool
    (PIL's decoders and numpy's file reads release the GIL): at ~800 frames/s of engine, one thread decoding a 1080p JPEG in ~10 ms
    would be the whole run (profiles/r5_cli_e2e.json: 62 frames/s with one thread, 333 with 8, 461 with 32).  SMAP_DECODE_THREADS
    (default: up to 16 of the allowed CPUs; 1 = decode in the consumer's thread, the round-4 behaviour).
    SMAP_DECODE_PROCS=<n>: the decoders as n WORKER PROCESSES (python -m dataset.decode: numpy + PIL only) writing into one shared-memory
    block, one slot per worker; the pool threads of this process then only talk to their worker and copy its slot into page-locked memory.
    What threads cannot scale past is the part of a decode that holds the interpreter lock (PIL's packers, file objects): ~600 frames/s on
    the bench's image mix, below the engine (EXPERIMENTS R6.11).  SMAP_DECODE_SLOT_MB (default 16): a larger frame is decoded in-thread.
    device_decode (`--device_decode 1`): the pool threads read the file bytes, parse the JPEG markers and Huffman-decode the coefficients
    into page-locked memory (native code, no interpreter lock); the consumer uploads them and the GPU finishes the decode (smap_amd/jpeg.py),
    bit for bit PIL's frame.  Whatever the native decoder does not take (progressive, PNG, damaged files ...) is decoded with PIL as before;
    the count is logged at the end of the run.  Worker processes (SMAP_DECODE_PROCS) are not used then.
    `--device_decode 2`: the Huffman decode runs on the GPU too (smap_amd/csrc/jpeg_huff.hip).  The pool threads only read the file, parse
    its markers and pack the scan's tables with the file bytes into one page-locked buffer; the consumer uploads it, launches the decode of
    every frame of the batch, waits ONCE per batch and reads the status words.  A frame the device decoder does not vouch for (status != 0)
    is decoded again by the host decoder, then by PIL, exactly as mode 1 would have decoded it; both counts are logged at the end.
    The dataset is asked path(i), name(i), geometry(i) (None: letter-box) and extras(i) (CustomDataset and JointDataset answer them, next
    to raw(i) for callers that want a frame with everything that belongs to it); the loader decodes path(i) itself, by whichever variant, and
    asks for geometry and extras in the same pool thread, ahead of the consumer.  For an annotated set (the ground-truth modes) a batch is what
    lib/utils/dataloader.py::collate_test yields: (imgs on the device, annotations [B,MAX_PEOPLE,15,C] fp32, tuple of paths, tuple of meta dicts)."""

    def __init__(self, dataset, indices, batch_size, cfg, device, device_decode=False):
        self.ds, self.idx, self.bs, self.cfg, self.device = dataset, list(indices), batch_size, cfg, device
        self.device_decode = bool(device_decode)
        self.device_huffman = int(device_decode) == 2        # --device_decode 2: the entropy decode on the GPU as well
        self.pil_frames = 0                                  # device_decode: frames that fell back to PIL
        self.host_frames = 0                                 # device_huffman: frames the host decoder redid
        try:
            allowed = len(os.sched_getaffinity(0))
        except AttributeError:
            allowed = os.cpu_count() or 1
        self.threads = int(os.environ.get("SMAP_DECODE_THREADS", "0")) or max(1, min(16, allowed))
        self.procs = int(os.environ.get("SMAP_DECODE_PROCS", "0"))
        if self.procs > 0 and self.device_decode:
            logging.getLogger(cfg.DATASET.NAME).info("SMAP_DECODE_PROCS=%d is not used with --device_decode 1", self.procs)
            self.procs = 0
        if self.procs > 0:
            self.threads = self.procs                        # one pool thread per worker process
        self.slot_bytes = int(os.environ.get("SMAP_DECODE_SLOT_MB", "16")) << 20

    def __len__(self):
        return (len(self.idx) + self.bs - 1) // self.bs

    def __iter__(self):
        yield from self._batches()
        if self.device_huffman:
            logging.getLogger(self.cfg.DATASET.NAME).info("device decode: {} of {} frames were redone on the host, {} fell back to PIL".format(
                self.host_frames, len(self.idx), self.pil_frames))
        elif self.device_decode:
            logging.getLogger(self.cfg.DATASET.NAME).info("device decode: {} of {} frames fell back to PIL".format(self.pil_frames, len(self.idx)))

    def _batches(self):
        self.pil_frames = self.host_frames = 0
        if self.threads <= 1:
            for s in range(0, len(self.idx), self.bs):
                idx = self.idx[s:s + self.bs]
                if self.device_huffman:
                    got = self._device_frames([self._coefficients(i, lambda img: img) for i in idx])
                elif self.device_decode:
                    got = [self._device_frame(self._coefficients(i, lambda img: img)) for i in idx]
                else:
                    got = [self._frame(i) for i in idx]
                yield self._batch(got, [self._rides_along(i) for i in idx])
            return
        import collections
        import contextlib
        from concurrent.futures import ThreadPoolExecutor
        ahead = max(2 * self.threads, 3 * self.bs)           # images being decoded or waiting: bounds the host memory (~6 MB per 1080p frame)

        def pinned(img):
            # ... leave the frame in PAGE-LOCKED memory (torch's caching host allocator recycles the blocks): the consumer's
            # upload is then an asynchronous DMA instead of a blocking pageable copy (~1 ms per 1080p frame of the consumer's time)
            buf = torch.empty(img.shape, dtype=torch.uint8, pin_memory=True)
            np.copyto(buf.numpy(), img)                      # (one copy, GIL released; `img` may be a read-only view of the decoder's bytes)
            return buf

        def decode(i):
            img, name = self._frame(i)
            return pinned(img), name
        workers = contextlib.ExitStack()
        if self.device_decode:
            def decode(i):
                return self._coefficients(i, pinned)
        elif self.procs > 0:
            decode = self._process_decoders(workers, pinned)
        with workers, ThreadPoolExecutor(self.threads) as ex:
            todo, futs = iter(self.idx), collections.deque()

            def fill():
                while len(futs) < ahead:
                    try:
                        i = next(todo)
                    except StopIteration:
                        return
                    futs.append(ex.submit(lambda i=i: (decode(i), self._rides_along(i))))
            fill()
            while futs:
                n = min(self.bs, len(futs))
                got, along = zip(*[futs.popleft().result() for _ in range(n)])     # in submission order: frame order is kept
                got = list(got)
                fill()
                if self.device_huffman:
                    got = self._device_frames(got)
                elif self.device_decode:
                    got = [self._device_frame(g) for g in got]
                yield self._batch(got, along)

    def _where(self, i):
        """(file, name in the records) of frame i: the dataset's path(i) and name(i).  The second branch serves ONE caller: a bare file list
        (image_list below dataset_path, no methods) handed to _process_decoders alone, as tests/test_entry_cpu.py does; nothing that yields
        batches works on such an object (geometry(i) and extras(i) are asked without a fallback)."""
        if hasattr(self.ds, "path"):
            return self.ds.path(i), self.ds.name(i)
        path = self.ds.image_list[i].rstrip()
        return path, path.replace(self.ds.dataset_path, "").lstrip("/")

    def _frame(self, i):
        """(frame i decoded in this thread, its name in the records): only the file is read, nothing of the annotations."""
        from dataset.decode import read_bgr
        path, name = self._where(i)
        return read_bgr(path), name

    def _rides_along(self, i):
        """(geometry, extras) of frame i: no file is touched; in the pool thread that decodes the frame."""
        return self.ds.geometry(i), self.ds.extras(i)

    def _batch(self, got, along):
        """Frames decoded as `got` = [(frame, name)] with `along` = [(geometry, extras)], as the batch the dataset's host loader would yield:
        one pre-processing launch (smap_amd/preprocess.py) on the dataset's geometry, then (imgs, names, scales) for an image folder (the
        default collate of CustomDataset's items) or (imgs, annotations, paths, metas) for an annotated set
        (lib/utils/dataloader.py::collate_test)."""
        from smap_amd.preprocess import preprocess_batch
        raws, names = zip(*got)
        geoms, extras = zip(*along)
        kw = {}
        if geoms[0] is not None:
            kw = dict(geometries=list(geoms), net_w=geoms[0][0]["net_width"], net_h=geoms[0][0]["net_height"])
        imgs, scales = preprocess_batch(raws, self.cfg.INPUT.MEANS, self.cfg.INPUT.STDS, self.device, **kw)
        if extras[0] is None:
            return imgs, list(names), scales
        annotations, metas = zip(*extras)
        return imgs, torch.stack(annotations, 0), tuple(names), tuple(metas)

    def _coefficients(self, i, pinned):
        """device_decode, in a pool thread: (("jpeg", coefficients in page-locked memory, info) or a PIL frame, name)."""
        from smap_amd import jpeg as J
        path, name = self._where(i)
        if not path.endswith(".npy"):
            with open(path, "rb") as f:
                data = f.read()
            info = J.probe(data)
            if self.device_huffman:
                frame = J.pack_frame(data, info) if info is not None else None
                if frame is not None:
                    return ("huff", frame, info, i), name
            coeffs = J.decode_coefficients(data, info) if info is not None and not self.device_huffman else None
            if coeffs is not None:
                return ("jpeg", coeffs, info), name
        return pinned(self._frame(i)[0]), name

    def _device_frame(self, item):
        """device_decode, in the consumer: upload the coefficients and finish the decode on the GPU (current stream)."""
        img, name = item
        if isinstance(img, tuple):
            from smap_amd import jpeg as J
            return J.reconstruct(img[1], img[2], self.device), name
        if not name.endswith(".npy"):
            self.pil_frames += 1
        return img, name

    def _device_frames(self, items):
        """device_huffman, in the consumer: upload every frame of the batch and launch its Huffman decode, wait once, read the status
        words; redo what the device does not vouch for as mode 1 does (host decoder, then PIL); finish the decode on the GPU."""
        from smap_amd import jpeg as J
        launched = [(k, J.decode_coefficients_device(img[1], img[2], None, self.device))
                    for k, (img, _) in enumerate(items) if isinstance(img, tuple)]
        status = torch.cat([st for _, (_, st) in launched]).cpu().tolist() if launched else []     # the one wait of the batch
        coeffs = {k: co for (k, (co, _)), st in zip(launched, status) if st == 0}
        out = []
        for k, (img, name) in enumerate(items):
            if isinstance(img, tuple) and k not in coeffs:
                self.host_frames += 1
                co = J.decode_coefficients(J.frame_bytes(img[1]), img[2])
                if co is None:
                    out.append(self._device_frame(self._frame(img[3])))
                    continue
                coeffs[k] = co
            if isinstance(img, tuple):
                out.append((J.reconstruct(coeffs[k], img[2], self.device), name))
            else:
                out.append(self._device_frame((img, name)))
        return out

    def _process_decoders(self, stack, pinned):
        """Start SMAP_DECODE_PROCS workers (dataset/decode.py) over one shared-memory block; -> decode(i) for the pool threads.  A pool
        thread takes a free worker and its slot per frame: it writes "<slot>\\t<path>", blocks on the answer (no interpreter lock held), copies the
        slot into page-locked memory.  `stack` closes the workers' pipes, waits for them and unlinks the block when the iteration ends."""
        import queue
        import subprocess
        import sys
        from multiprocessing import shared_memory
        root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        shm = shared_memory.SharedMemory(create=True, size=self.procs * self.slot_bytes)
        view = np.frombuffer(shm.buf, np.uint8)
        procs = [subprocess.Popen([sys.executable, "-m", "dataset.decode", shm.name, str(self.slot_bytes)], cwd=root, text=True, bufsize=1,
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=dict(os.environ, OMP_NUM_THREADS="1"))
                 for _ in range(self.procs)]
        free = queue.Queue()
        for k in range(self.procs):
            free.put(k)

        def close():
            nonlocal view
            for p in procs:
                try:
                    p.stdin.close()
                except Exception:
                    pass
            for p in procs:
                try:
                    p.wait(timeout=5)
                except Exception:
                    p.kill()
            view = None
            shm.close()
            shm.unlink()
        stack.callback(close)

        def decode(i):
            k = free.get()                                   # a worker and its slot, for this frame (as many pool threads as workers: no wait)
            try:
                p = procs[k]
                path, name = self._where(i)
                path = os.path.abspath(path)                 # the workers run in another directory
                p.stdin.write(f"{k}\t{path}\n")
                p.stdin.flush()
                ans = p.stdout.readline().split(None, 3)
                if len(ans) < 3:
                    raise RuntimeError(f"decode worker {k} died on {path}")
                h, w = int(ans[1]), int(ans[2])
                if h == -1:                                  # larger than a slot: here, in this thread
                    return pinned(self._frame(i)[0]), name
                if h < 0:
                    raise RuntimeError(f"decode worker: {path}: {ans[3] if len(ans) > 3 else 'failed'}")
                n = h * w * 3
                return pinned(view[k * self.slot_bytes:k * self.slot_bytes + n].reshape(h, w, 3)), name
            finally:
                free.put(k)
        return decode


class AnnotationLoader:
    """`--maps_from_gt 1`: batches of an annotated set WITHOUT its images -- (None, annotations [B,MAX_PEOPLE,15,C] fp32, tuple of names,
    tuple of meta dicts), the batch of lib/utils/dataloader.py::collate_test with no frames in it.  Only dataset.extras(i) and name(i)
    are asked: no file is opened."""

    def __init__(self, dataset, indices, batch_size):
        self.ds, self.idx, self.bs = dataset, list(indices), batch_size

    def __len__(self):
        return (len(self.idx) + self.bs - 1) // self.bs

    def __iter__(self):
        for s in range(0, len(self.idx), self.bs):
            idx = self.idx[s:s + self.bs]
            annotations, metas = zip(*[self.ds.extras(i) for i in idx])
            yield None, torch.stack(annotations, 0), tuple(self.ds.name(i) for i in idx), tuple(metas)


class _DryRunPipeline:
    """Stand-in for PosePipeline in `--dry_run 1` (no GPU, no checkpoint): the same submit / flush contract -- records of
    the batch submitted `depth` calls earlier -- with one fake person per frame.  What the rehearsal exercises is everything
    AROUND the device work: CLI, image listing, the contiguous per-rank split, ragged last batches, the end-of-run gather
    (gloo instead of RCCL) and the result file; `python -m torch.distributed.run --nproc-per-node 8 test.py --dry_run 1 ...`."""

    def __init__(self, model, cfg, batch, H, W, device, refine_w=None, depth=2, **kw):
        self.B, self.depth, self.q = batch, max(1, int(depth)), []

    def submit(self, imgs, cams, tags, annotations=None):
        from smap_amd.records import frame_record
        p2 = np.zeros((1, 15, 4), np.float32)
        self.q.append([frame_record(p2, np.zeros((1, 15, 4)), np.full((1,), float(imgs[i].mean())), t, None, as_lists=False)
                       for i, t in enumerate(tags) if t is not None])
        return self.q.pop(0) if len(self.q) > self.depth else None

    def flush(self):
        out = [r for recs in self.q for r in recs]
        self.q = []
        return out or None


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

    import time
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
        annotations = None
        if cfg.TEST_MODE == "run_inference":
            imgs, img_path, scales = batch
            cams = default_cams(scales, len(imgs))
        else:                                                    # test.py:50-51,73-95
            imgs, meta_data, img_path, scales = batch
            annotations = [kept_annotations(m.numpy(), cfg.DATASET.ROOT_IDX) for m in meta_data]
            cams = [annotation_camera(a, s) if len(a) else [1.0] * 9 for a, s in zip(annotations, scales)]
        img_path = list(img_path)
        map_inputs = None
        if maps_from_gt:
            n, pad = len(img_path), (pipe.B - len(img_path) if pipe is not None else 0)
            all_annotations = list(meta_data) + [meta_data[-1]] * max(pad, 0)      # a ragged last batch repeats its last frame (tag None)
            map_inputs = (all_annotations, list(scales) + [scales[-1]] * max(pad, 0))
            if pad > 0:
                cams = np.concatenate([np.asarray(cams, np.float64), np.repeat(np.asarray(cams, np.float64)[-1:], pad, 0)], 0)
                img_path = img_path + [None] * pad
                annotations = list(annotations) + [annotations[-1]] * pad
            imgs = _NoFrames(len(img_path), cfg.dataset.INPUT_SHAPE)
        else:
            imgs = imgs.to(device, non_blocking=True).float().contiguous()
        if val_loss is not None:                                 # before the padding: the batch's real frames, unmirrored, a forward of its own
            val_loss.update(imgs, meta_data, scales)
        if not maps_from_gt and pipe is not None and len(imgs) < pipe.B:              # ragged last batch: pad with copies of its last frame and
            pad = pipe.B - len(imgs)                             # drop their records (tag None) -- no second engine / arena
            imgs = torch.cat([imgs, imgs[-1:].expand(pad, -1, -1, -1)], 0).contiguous()
            cams = np.concatenate([np.asarray(cams, np.float64), np.repeat(np.asarray(cams, np.float64)[-1:], pad, 0)], 0)
            img_path = img_path + [None] * pad
            if annotations is not None:
                annotations = list(annotations) + [annotations[-1]] * pad
        if pipe is None or pipe.B != len(imgs):
            if pipe is not None:
                retire(pipe)
            pipe = pipeline_cls(model, cfg, len(imgs), imgs.shape[-2], imgs.shape[-1], device, refine_w,
                                do_flip=bool(cfg.DO_FLIP), record_mode=cfg.TEST_MODE, numpy_records=True,
                                depth=int(os.environ.get("SMAP_PIPELINE_DEPTH", 2)),   # two backbones in flight (+19 %)
                                **evaluators, **source)
        with torch.no_grad():
            if maps_from_gt:
                drain(pipe.submit(None, cams, list(img_path), annotations=annotations, map_inputs=map_inputs))
            else:
                drain(pipe.submit(imgs, cams, list(img_path), annotations=annotations))
        clock["submit_s"] += time.perf_counter() - t_sub
        if "first_submit_s" not in clock:                        # builds the engine (schedule, weight packing, plan, arenas): seconds, once
            clock["first_submit_s"] = time.perf_counter() - t_sub
        clock["frames"] += sum(1 for p_ in img_path if p_ is not None)
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
    if dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("SMAP_FORCE_GATHER", "") == "1"):
        parts = gather_records(result["3d_pairs"], device)
        result["3d_pairs"] = [r for part in parts for r in part]                # rank order == frame order
        dropped = [n for part in gather_records(dropped, device) for n in part]
    if dropped:
        # the reference's fp32 forward has no such failure: say so where the caller will look (the result file and the exit status)
        result["dropped_frames"] = list(dropped)
        logger.warning("{} frame(s) have no result (non-finite maps: an activation exceeded the fp16 range, INTEGRATION.md section 5): {}".format(
            len(dropped), dropped[:20]))
    for ev in evaluators.values():
        raw = ev.raw()                                                          # the run's only read-back of the scores
        if dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("SMAP_FORCE_GATHER", "") == "1"):
            raw = ev.merge_raws(gather_records(raw, device))                    # rank order; evaluate.merge / merge_maps say what that costs
        if rank == 0:
            for line in ev.log_lines(raw):                                      # calculate_and_log's lines (test_util_panoptic.py:388-400, :374-378)
                logger.info(line)
            result.setdefault("error", {}).update(ev.result_entry(raw))
    if val_loss is not None:
        raw = val_loss.raw()                                                    # one read-back
        if dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("SMAP_FORCE_GATHER", "") == "1"):
            raw = val_loss.merge_raws(gather_records(raw, device))
        if rank == 0:
            entry = val_loss.result_entry(raw)
            logger.info("validation loss over {frames} frames in {batches} batches: total {total_loss:.6g}  2d {loss_2d:.6g}  bone {loss_bone:.6g}  "
                        "root {loss_root:.6g}".format(**entry["loss"]))
            result.setdefault("error", {}).update(entry)
    if rank == 0:
        dir_name = os.path.split(os.path.split(os.path.realpath(__file__))[0])[1]
        name = os.path.join(output_dir, "{}_{}_{}_{}.json".format(dir_name, cfg.TEST_MODE, cfg.DATA_MODE,
                                                                  cfg.JSON_SUFFIX_NAME))
        result["3d_pairs"] = to_jsonable(result["3d_pairs"])          # ndarray -> nested lists, once, at the end of the run
        mupots_refusal = None
        if mupots_ann is not None:                                    # on the records as the file will hold them
            from lib.eval.convert import convert_records
            from smap_amd.mupots import MuPoTSScorer
            try:
                pose3d, pose2d, _ = convert_records(result["3d_pairs"])
                summary = MuPoTSScorer(mupots_ann, device=device).score(pose2d, pose3d).summary()
                logger.info("MuPoTS-3D: 3DPCK {mean_pck:.4g}  AUC {mean_auc:.4g}  MPJPE {mean_mpjpe:.6g} mm (means over the sequences)".format(**summary))
                result.setdefault("error", {})["mupots"] = summary
            except Exception as exc:                                  # refused or failed: the pairs are written all the same
                mupots_refusal = exc
        with open(name, "w") as f:
            json.dump(result, f)
        logger.info("Pairs writed to {}".format(name))
        if mupots_refusal is not None:
            raise mupots_refusal
    return result


class _NoFrames:
    """What the loop reads of a batch of frames (its length and shape) when there are none (--maps_from_gt 1)."""

    def __init__(self, n, input_shape):
        self.shape = (n, 3, int(input_shape[0]), int(input_shape[1]))

    def __len__(self):
        return self.shape[0]


def main():
    # the schedule of a (checkpoint, shape, arithmetic) is built once and kept on disk (smap_amd/engine.py plan cache): the second start of
    # this command loads it through smap_plan_create_from_blob instead of re-packing the weights (SMAP_PLAN_CACHE=0 switches it off)
    os.environ.setdefault("SMAP_PLAN_CACHE", os.path.join(os.environ.get("XDG_CACHE_HOME", os.path.expanduser("~/.cache")), "smap_amd"))
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
    args = parser.parse_args()
    if args.eval_mupots and args.test_mode != "generate_result":
        parser.error("--eval_mupots requires -t generate_result")
    if args.eval_mupots and args.dry_run:
        parser.error("--eval_mupots scores on the GPU: not available with --dry_run 1")
    if args.eval_loss and args.test_mode != "generate_result":
        parser.error("--eval_loss 1 requires -t generate_result")
    if args.eval_loss and args.dry_run:
        parser.error("--eval_loss 1 runs on the GPU: not available with --dry_run 1")
    if args.eval_loss and args.maps_from_gt:
        parser.error("--eval_loss 1 needs the network's heads: not available with --maps_from_gt 1")
    if args.maps_from_gt and args.test_mode == "run_inference":
        parser.error("--maps_from_gt 1 renders the maps from annotations: -t run_inference has none (use -t generate_result or generate_train)")
    if args.maps_from_gt and args.dry_run:
        parser.error("--maps_from_gt 1 renders on the GPU: not available with --dry_run 1")
    if args.device_decode not in (0, 1, 2):
        parser.error("--device_decode is 0, 1 or 2")
    if args.device_decode and not args.device_preprocess:
        parser.error("--device_decode {} requires --device_preprocess 1".format(args.device_decode))
    if args.eval_3d and args.test_mode != "generate_result":
        parser.error("--eval_3d 1 requires -t generate_result")
    if args.eval_3d and args.dry_run:
        parser.error("--eval_3d 1 scores on the GPU: not available with --dry_run 1")
    if args.eval_maps and args.test_mode != "generate_result":
        parser.error("--eval_maps 1 requires -t generate_result")
    if args.eval_maps and args.dry_run:
        parser.error("--eval_maps 1 scores on the GPU: not available with --dry_run 1")
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
        from smap_amd.dist import init_single_rank_group       # one rank, real collectives: the RCCL path on a one-GPU box (tests)
        init_single_rank_group("gloo" if dry else "nccl")
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

    if args.test_mode != "run_inference" and args.device_preprocess and dry:
        logger.info("--dry_run 1: the ground-truth modes are rehearsed on the host loader (--device_preprocess needs the GPU)")
    if args.maps_from_gt:
        from dataset.base_dataset import JointDataset
        from lib.utils.dataloader import rank_block
        if cfg.DATASET.NAME != "MIX":                          # get_test_loader's check
            raise NameError("Dataset is not defined!", cfg.DATASET.NAME)
        dataset = JointDataset(cfg, args.data_mode)
        if args.device_preprocess:
            logger.info("--maps_from_gt 1: no frame is read, --device_preprocess / --device_decode are ignored")
        data_loader = AnnotationLoader(dataset, range(*rank_block(len(dataset), world, dist.get_rank() if world > 1 else 0)), args.batch_size)
        dataset = None
    elif args.test_mode != "run_inference" and args.device_preprocess and not dry:
        from dataset.base_dataset import JointDataset
        from lib.utils.dataloader import rank_block
        if cfg.DATASET.NAME != "MIX":                          # get_test_loader's check
            raise NameError("Dataset is not defined!", cfg.DATASET.NAME)
        dataset = JointDataset(cfg, args.data_mode)
        indices = range(*rank_block(len(dataset), world, dist.get_rank() if world > 1 else 0))      # get_test_loader's split
    elif args.test_mode != "run_inference":
        from lib.utils.dataloader import get_test_loader
        data_loader = get_test_loader(cfg, num_gpu=world, local_rank=dist.get_rank() if world > 1 else 0,
                                      stage=args.data_mode)
        dataset = indices = None
    else:
        dataset = CustomDataset(cfg, args.dataset_path)
        indices = range(len(dataset))
        if world > 1:
            st, ed = shard_range(len(dataset), world, dist.get_rank())
            indices = range(st, ed)
    if dataset is None:
        pass
    elif args.device_preprocess:
        data_loader = DevicePreprocLoader(dataset, indices, args.batch_size, cfg, torch.device(cfg.MODEL.DEVICE, local),
                                          device_decode=args.device_decode)
    else:
        data_loader = DataLoader(Subset(dataset, indices) if world > 1 else dataset, batch_size=args.batch_size,
                                 shuffle=False)

    if dry:
        generate_3d_point_pairs(None, None, data_loader, cfg, logger, device, output_dir=os.path.join(cfg.OUTPUT_DIR, "result"),
                                pipeline_cls=_DryRunPipeline)
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
