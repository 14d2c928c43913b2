"""The batch loaders of the entry script (exps/stage3_root2/test.py): DevicePreprocLoader (`--device_preprocess 1 [--device_decode 1|2]`:
frames decoded ahead of the consumer, resized / padded / normalised on the GPU) and AnnotationLoader (`--maps_from_gt 1`: annotations, no frames);
and the training side: TrainSet + TrainLoader (lib/utils/dataloader.py::get_train_loader), whose batches are augmented and labelled on the GPU."""
import collections
import contextlib
import functools
import json
import logging
import os
import queue
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from multiprocessing import shared_memory

import numpy as np
import torch

from dataset.decode import read_bgr
from .augment import AugParams, augment_batch, draw, plan_sample
from .labels import label_spec, render_labels, root_depth_labels, valid_vector
from .preprocess import preprocess_batch


def pinned(img):
    """A decoded frame in PAGE-LOCKED memory (torch's caching host allocator recycles the blocks): the consumer's upload is then an
    asynchronous DMA instead of a blocking pageable copy (~1 ms per 1080p frame of the consumer's time)."""
    buf = torch.empty(img.shape, dtype=torch.uint8, pin_memory=True)
    np.copyto(buf.numpy(), img)                              # (one copy, GIL released; `img` may be a read-only view of the decoder's bytes)
    return buf


class DevicePreprocLoader:
    """Batches of (imgs on the device, names, scales) with decode on the host and resize / pad /
    normalise in one HIP launch per batch of up to 16 frames (smap_amd/preprocess.py: smap_preprocess_batch).  The decodes run AHEAD of the consumer on a small thread pool
    (PIL's decoders and numpy's file reads release the GIL): at ~800 frames/s of engine, one thread decoding a 1080p JPEG in ~10 ms
    would be the whole run (profiles/r5_cli_e2e.json: 62 frames/s with one thread, 333 with 8, 461 with 32).  SMAP_DECODE_THREADS
    (default: up to 16 of the allowed CPUs; 1 = decode in the consumer's thread, batch by batch, no thread started).
    SMAP_DECODE_PROCS=<n>: the decoders as n WORKER PROCESSES (process_decoders below) writing into one shared-memory
    block, one slot per worker; the pool threads of this process then only talk to their worker and copy its slot into page-locked memory.
    What threads cannot scale past is the part of a decode that holds the interpreter lock (PIL's packers, file objects): ~600 frames/s on
    the bench's image mix, below the engine (EXPERIMENTS R6.11).  SMAP_DECODE_SLOT_MB (default 16): a larger frame is decoded in-thread.
    A decode VARIANT is a pair: what a pool thread does for frame i -> (item, name), and what the consumer does with a batch of those
    -> [(frame, name)]; __init__ picks the pair, the walk (_batches) calls it.
    PIL (_pil_frame, nothing): the thread decodes the file (dataset/decode.py: read_bgr), or hands it to its worker process.
    `--device_decode 1` (_host_huffman, _reconstruct): the pool threads read the file bytes, parse the JPEG markers and Huffman-decode
    the coefficients into page-locked memory (native code, no interpreter lock); the consumer uploads them and the GPU finishes the decode
    (smap_amd/jpeg.py), bit for bit PIL's frame.  Whatever the native decoder does not take (progressive, PNG, damaged files ...) is
    decoded with PIL as before; the count is logged at the end of the run.  Worker processes (SMAP_DECODE_PROCS) are not used then.
    `--device_decode 2` (_packed_file, _device_huffman): the Huffman decode runs on the GPU too (smap_amd/csrc/jpeg_huff.hip).  The pool
    threads only read the file, parse its markers and pack the scan's tables with the file bytes into one page-locked buffer; the consumer
    uploads it, launches the decode of every frame of the batch, waits ONCE per batch and reads the status words.  A frame the device
    decoder does not vouch for (status != 0) is decoded again by the host decoder, then by PIL, exactly as mode 1 would have decoded it;
    both counts are logged at the end.
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
        self.threads = int(os.environ.get("SMAP_DECODE_THREADS", "0")) or max(1, min(16, len(os.sched_getaffinity(0))))
        self.procs = int(os.environ.get("SMAP_DECODE_PROCS", "0"))
        if self.procs > 0 and self.device_decode:
            logging.getLogger(cfg.DATASET.NAME).info("SMAP_DECODE_PROCS=%d is not used with --device_decode 1", self.procs)
            self.procs = 0
        if self.procs > 0:
            self.threads = self.procs                        # one pool thread per worker process
        self.slot_bytes = int(os.environ.get("SMAP_DECODE_SLOT_MB", "16")) << 20
        self._in_thread, self._in_consumer = ((self._packed_file, self._device_huffman) if self.device_huffman else
                                              (self._host_huffman, self._reconstruct) if self.device_decode else (self._pil_frame, list))

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
        """The one walk.  With a pool, max(2 * threads, 3 * batch) frames are being decoded or waiting (bounds the host memory: ~6 MB per
        1080p frame); without one (SMAP_DECODE_THREADS=1) the same queue holds calls not yet made: a frame is decoded when its batch is due."""
        self.pil_frames = self.host_frames = 0
        pooled = self.threads > 1
        ahead = max(2 * self.threads, 3 * self.bs)
        pin = pinned if pooled else (lambda img: img)
        with contextlib.ExitStack() as stack:
            decode = functools.partial(self._in_thread, pin=pin)
            if pooled and self.procs > 0:
                decode = process_decoders(stack, self.ds, self.procs, self.slot_bytes, pin)

            def job(i):                                      # (frame i by the variant, name), (geometry, extras): no file is touched for the latter
                return decode(i), (self.ds.geometry(i), self.ds.extras(i))
            if pooled:
                pool = stack.enter_context(ThreadPoolExecutor(self.threads))
                start = lambda i: pool.submit(job, i).result
            else:
                start = lambda i: functools.partial(job, i)
            todo, due = iter(self.idx), collections.deque()

            def fill():
                while len(due) < ahead:
                    try:
                        due.append(start(next(todo)))
                    except StopIteration:
                        return
            fill()
            while due:
                got, along = zip(*[due.popleft()() for _ in range(min(self.bs, len(due)))])     # in submission order: frame order is kept
                fill()
                yield self._batch(self._in_consumer(got), along)

    def _batch(self, got, along):
        """Frames decoded as `got` = [(frame, name)] with `along` = [(geometry, extras)], as the batch the dataset's host loader would yield:
        one pre-processing launch (smap_amd/preprocess.py) on the dataset's geometry, then (imgs, names, scales) for an image folder (the
        default collate of CustomDataset's items) or (imgs, annotations, paths, metas) for an annotated set
        (lib/utils/dataloader.py::collate_test)."""
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

    # ---- the decode variants: in a pool thread, frame i -> (item, name); in the consumer, items of a batch -> [(frame, name)] ----
    def _pil_frame(self, i, pin):
        """(frame i decoded in this thread, its name in the records): only the file is read, nothing of the annotations."""
        return pin(read_bgr(self.ds.path(i))), self.ds.name(i)

    def _probed(self, i):
        """(file bytes, JpegInfo) of frame i when the native decoder takes the file, else (None, None)."""
        from smap_amd import jpeg as J
        path = self.ds.path(i)
        if path.endswith(".npy"):
            return None, None
        with open(path, "rb") as f:
            data = f.read()
        info = J.probe(data)
        return (data, info) if info is not None else (None, None)

    def _host_huffman(self, i, pin):
        """(("jpeg", coefficients in page-locked memory, info) or a PIL frame, name)."""
        from smap_amd import jpeg as J
        data, info = self._probed(i)
        coeffs = J.decode_coefficients(data, info) if info is not None else None
        return (("jpeg", coeffs, info), self.ds.name(i)) if coeffs is not None else self._pil_frame(i, pin)

    def _counted(self, item):
        """A frame that reached the consumer decoded by PIL although a device decode was asked for."""
        if not item[1].endswith(".npy"):
            self.pil_frames += 1
        return item

    def _reconstruct(self, items):
        """Upload the coefficients and finish the decode on the GPU (current stream)."""
        from smap_amd import jpeg as J
        return [(J.reconstruct(img[1], img[2], self.device), name) if isinstance(img, tuple) else self._counted((img, name)) for img, name in items]

    def _packed_file(self, i, pin):
        """(("huff", scan tables + file bytes in one page-locked buffer, info, i) or a PIL frame, name)."""
        from smap_amd import jpeg as J
        data, info = self._probed(i)
        frame = J.pack_frame(data, info) if info is not None else None
        return (("huff", frame, info, i), self.ds.name(i)) if frame is not None else self._pil_frame(i, pin)

    def _device_huffman(self, items):
        """Upload every frame of the batch and launch its Huffman decode, wait once, read the status words; redo what the device does
        not vouch for as mode 1 does (host decoder, then PIL); finish the decode on the GPU."""
        from smap_amd import jpeg as J
        launched = [(k, J.decode_coefficients_device(img[1], img[2], None, self.device))
                    for k, (img, _) in enumerate(items) if isinstance(img, tuple)]
        status = torch.cat([st for _, (_, st) in launched]).cpu().tolist() if launched else []     # the one wait of the batch
        coeffs = {k: co for (k, (co, _)), st in zip(launched, status) if st == 0}
        out = []
        for k, (img, name) in enumerate(items):
            if isinstance(img, tuple) and k not in coeffs:
                self.host_frames += 1
                coeffs[k] = J.decode_coefficients(J.frame_bytes(img[1]), img[2])
            if not isinstance(img, tuple):
                out.append(self._counted((img, name)))
            elif coeffs[k] is None:
                out.append(self._counted(self._pil_frame(img[3], lambda a: a)))
            else:
                out.append((J.reconstruct(coeffs[k], img[2], self.device), name))
        return out


def process_decoders(stack, dataset, procs, slot_bytes, pin):
    """Start `procs` workers (dataset/decode.py) over one shared-memory block of `procs` slots; -> decode(i) -> (pin(frame), name) for
    the pool threads.  A pool thread takes a free worker and its slot per frame: it writes "<slot>\\t<path>", blocks on the answer (no
    interpreter lock held), copies the slot out with `pin`.  `stack` (a contextlib.ExitStack) closes the workers' pipes, waits for them
    and unlinks the block when the iteration ends."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shm = shared_memory.SharedMemory(create=True, size=procs * slot_bytes)
    view = np.frombuffer(shm.buf, np.uint8)
    workers = [subprocess.Popen([sys.executable, "-m", "dataset.decode", shm.name, str(slot_bytes)], cwd=root, text=True, bufsize=1,
                                stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=dict(os.environ, OMP_NUM_THREADS="1"))
               for _ in range(procs)]
    free = queue.Queue()
    for k in range(procs):
        free.put(k)

    def close():
        nonlocal view
        for p in workers:
            try:
                p.stdin.close()
            except Exception:
                pass
        for p in workers:
            try:
                p.wait(timeout=5)
            except Exception:
                p.kill()
        view = None
        shm.close()
        shm.unlink()
    stack.callback(close)

    def decode(i):
        k = free.get()                                       # a worker and its slot, for this frame (as many pool threads as workers: no wait)
        try:
            p, name = workers[k], dataset.name(i)
            path = os.path.abspath(dataset.path(i))          # the workers run in another directory
            p.stdin.write(f"{k}\t{path}\n")
            p.stdin.flush()
            ans = p.stdout.readline().split(None, 3)
            if len(ans) < 3:
                raise RuntimeError(f"decode worker {k} died on {path}")
            h, w = int(ans[1]), int(ans[2])
            if h == -1:                                      # larger than a slot: here, in this thread
                return pin(read_bgr(path)), name
            if h < 0:
                raise RuntimeError(f"decode worker: {path}: {ans[3] if len(ans) > 3 else 'failed'}")
            return pin(view[k * slot_bytes:k * slot_bytes + h * w * 3].reshape(h, w, 3)), name
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


class TrainSet:
    """The annotation records of stage `train` (reference: dataset/base_dataset.py:32-56,65-66): the COCO JSON with every set of
    USED_3D_DATASETS put in front of it, entries with isValidation == 0; a frame lies under its own dataset's root path.
    A sample key is (epoch, index), or a bare index (epoch 0): its five draws come from a random.Random seeded with (seed, epoch,
    index), so a sample does not depend on which pool thread plans it, nor on the batch it falls into.  It answers what
    DevicePreprocLoader asks of a dataset: path / name / geometry (the image plan of smap_amd.augment.plan_sample) / extras
    ((bodys [P,15,C] float64 in network pixels, valid [57,1], meta)); no file is opened for the latter two."""

    def __init__(self, cfg, with_augmentation=True, seed=0, data=None):
        ds = cfg.dataset
        if data is None:
            with open(ds.COCO_JSON_PATH) as f:
                data = json.load(f)["root"]
            for name in ds.USED_3D_DATASETS:
                with open(ds["%s_JSON_PATH" % name]) as f:
                    data = json.load(f)["root"] + data
        self.data = [d for d in data if d["isValidation"] == 0]
        self.root_path = {name: ds["%s_ROOT_PATH" % name] for name in ["COCO"] + list(ds.USED_3D_DATASETS) if ("%s_ROOT_PATH" % name) in ds}
        self.params = AugParams.from_cfg(cfg)
        self.with_augmentation, self.seed = bool(with_augmentation), seed

    def __len__(self):
        return len(self.data)

    @staticmethod
    def _key(key):
        return (0, int(key)) if isinstance(key, (int, np.integer)) else (int(key[0]), int(key[1]))

    def path(self, key):
        d = self.data[self._key(key)[1]]
        return os.path.join(self.root_path[d["dataset"].upper()], d["img_paths"])

    def name(self, key):
        return self.data[self._key(key)[1]]["img_paths"]

    def plan(self, key):
        """(bodys, meta, fields) of smap_amd.augment.plan_sample for sample `key`."""
        epoch, index = self._key(key)
        rng = random.Random("%s:%d:%d" % (self.seed, epoch, index))
        return plan_sample(self.data[index], draw(rng), self.params, self.with_augmentation)

    def geometry(self, key):
        return self.plan(key)[2]

    def extras(self, key):
        bodys, meta, _ = self.plan(key)
        return bodys, valid_vector(meta["dataset"]), meta


class TrainLoader(DevicePreprocLoader):
    """Training batches on the device, in the shapes of the reference's BatchCollator (lib/utils/dataloader.py:48-58):
    (imgs [B,3,H,W], valids [B,57,1], labels [B,S,57,H/4,W/4], rdepth [B,MAX_PEOPLE,3]), all fp32 on `device` -- what
    SMAP.forward(imgs, valids, labels, rdepth) and SMAPLoss consume.  The decode-ahead walk, the page-locked uploads and the decode
    variants are DevicePreprocLoader's, unchanged; a batch is one smap_augment_batch launch (smap_amd/augment.py) on the planned
    geometry and the label renderer's two launches (smap_amd/labels.py) on the planned key points.  dataset: a TrainSet; indices: its
    sample keys."""

    def __init__(self, dataset, indices, batch_size, cfg, device, device_decode=False, with_mds=False):
        super().__init__(dataset, indices, batch_size, cfg, device, device_decode)
        self.spec, self.with_mds = label_spec(cfg), bool(with_mds)

    def _batch(self, got, along):
        raws, _ = zip(*got)
        plans, extras = zip(*along)
        bodys, valids, metas = zip(*extras)
        net_h, net_w = self.cfg.dataset.INPUT_SHAPE
        imgs = augment_batch(raws, plans, self.cfg.INPUT.MEANS, self.cfg.INPUT.STDS, self.device, net_w=net_w, net_h=net_h)
        labels = render_labels(list(bodys), self.spec, self.with_mds, self.device)
        rdepth = np.stack([root_depth_labels(b, m["scale"], self.spec) for b, m in zip(bodys, metas)])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device, non_blocking=True)
        return imgs, to(np.stack(valids)), labels, to(rdepth)
