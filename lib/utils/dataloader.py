"""Test-time data loading for the ground-truth modes (reference: lib/utils/dataloader.py:68-113).

`get_test_loader(cfg, num_gpu, local_rank, stage)`: the annotated dataset split in contiguous blocks of
ceil(N / num_gpu) frames per rank (dataloader.py:80-85), read sequentially in batches of cfg.TEST.IMG_PER_GPU;
a batch is (images [B,3,512,832], annotations [B,MAX_PEOPLE,15,C], tuple of image paths, tuple of scale dicts)
(BatchCollator, dataloader.py:98-106).
`get_train_loader(...)`: the training batches (dataloader.py:11-65), decoded ahead on the host, augmented and labelled on the GPU
(smap_amd/loaders.py::TrainLoader)."""
import math

import torch
from torch.utils.data import DataLoader, Subset

from dataset.base_dataset import JointDataset


def collate_test(batch):
    images, meta, paths, scales = zip(*batch)
    return torch.stack(images, 0), torch.stack(meta, 0), tuple(paths), tuple(scales)


def rank_block(n, num_gpu, rank):
    """[start, end) of rank `rank`: contiguous blocks of ceil(n / num_gpu) frames (dataloader.py:80-85); the last ranks may get fewer
    frames, or none (start == end)."""
    per = math.ceil(n / num_gpu)
    st = min(n, rank * per)
    return st, min(n, st + per)


def get_test_loader(cfg, num_gpu, local_rank, stage, use_augmentation=False, with_mds=False):
    if cfg.DATASET.NAME != "MIX":
        raise NameError("Dataset is not defined!", cfg.DATASET.NAME)
    dataset = JointDataset(cfg, stage, None, use_augmentation, with_mds)
    st, ed = rank_block(len(dataset), num_gpu, local_rank)
    workers = int(cfg.get("DATALOADER", {}).get("NUM_WORKERS", 0)) if hasattr(cfg, "get") else 0
    return DataLoader(Subset(dataset, range(st, ed)), batch_size=cfg.TEST.IMG_PER_GPU, shuffle=False, drop_last=False,
                      num_workers=workers, collate_fn=collate_test)


def train_batches(n, num_replicas, rank, batch_size, max_iter, start_iter=0, shuffle=True):
    """The sample keys of one rank's training run: a list of max_iter - start_iter batches, each a list of batch_size keys
    (epoch, index).  Epoch e visits the n samples in the order of torch.randperm under a generator seeded with e (in file order without
    shuffle); rank r takes every num_replicas-th sample from the r-th on, so the ranks of an epoch are disjoint; batches run on
    across epoch ends, so every batch is full.  Batch i is the same whatever start_iter is: a resumed run continues the stream."""
    if n <= 0 or batch_size <= 0 or not 0 <= rank < num_replicas:
        raise ValueError("train_batches: n, batch_size > 0 and 0 <= rank < num_replicas")
    orders = {}

    def order(epoch):
        if epoch not in orders:
            if shuffle:
                g = torch.Generator()
                g.manual_seed(epoch)
                full = torch.randperm(n, generator=g).tolist()
            else:
                full = list(range(n))
            orders.clear()                                   # (one epoch's order at a time)
            orders[epoch] = full[rank::num_replicas]
        return orders[epoch]
    per = len(range(rank, n, num_replicas))
    if per == 0:
        raise ValueError("train_batches: rank %d of %d has no sample among %d" % (rank, num_replicas, n))
    out = []
    for it in range(start_iter, max_iter):
        keys = []
        for pos in range(it * batch_size, (it + 1) * batch_size):
            epoch = pos // per
            keys.append((epoch, order(epoch)[pos - epoch * per]))
        out.append(keys)
    return out


def get_train_loader(cfg, num_gpu, is_dist=True, is_shuffle=True, start_iter=0, use_augmentation=True, with_mds=False, dataset=None,
                     rank=None, device=None):
    """The reference's signature (lib/utils/dataloader.py:11), plus three optional arguments: a TrainSet to use instead of reading the
    annotation files, the rank (default: the process group's) and the device (default: the current one).  Yields
    cfg.SOLVER.MAX_ITER - start_iter batches of cfg.SOLVER.IMG_PER_GPU samples, (imgs, valids, labels, rdepth) on the device.
    The ORDER is this project's own (train_batches): the reference's samplers are unseeded (RandomSampler; DistributedSampler
    reshuffles by an epoch nobody sets), so there is no order of theirs to reproduce.  With is_dist the num_gpu ranks take disjoint
    strides of every epoch; without it this process sees every sample."""
    from lib.utils.comm import get_rank
    from smap_amd.loaders import TrainLoader, TrainSet
    if cfg.DATASET.NAME != "MIX":
        raise NameError("Dataset is not defined!", cfg.DATASET.NAME)
    dataset = TrainSet(cfg, use_augmentation) if dataset is None else dataset
    replicas = int(num_gpu) if is_dist else 1
    rank = (get_rank() if is_dist else 0) if rank is None else int(rank)
    batch = int(cfg.SOLVER.IMG_PER_GPU)
    keys = [k for b in train_batches(len(dataset), replicas, rank, batch, int(cfg.SOLVER.MAX_ITER), start_iter, is_shuffle) for k in b]
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda:0")
    return TrainLoader(dataset, keys, batch, cfg, device, with_mds=with_mds)
