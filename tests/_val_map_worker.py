"""One rank of the two-rank multi-label validation epoch (tests/test_eval_metrics_gpu.py): RANK / WORLD_SIZE /
MASTER_PORT from the environment as tests/_ddp_worker.py takes them.  Every rank appends ITS OWN rows of the seeded
epoch — batch i of the epoch goes to rank i % world — to a DeviceValMeter with NUM_GPUS = world, logs the epoch and
leaves {"map", "host_reads", "cap", "rows"} in <out_dir>/valmap_rank<r>.json.

usage: _val_map_worker.py <out_dir> [backend [device]]   (default: nccl on device RANK; "gloo 0" puts every rank on
device 0, which RCCL refuses)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SEED, MAX_ITER, MB, NCLS = 31, 3, 5, 9  # per rank: 3 batches of 5 rows


def epoch_rows(world):
    """The whole epoch: preds / labels float32 [world * MAX_ITER * MB, NCLS]."""
    rs = np.random.RandomState(SEED)
    n = world * MAX_ITER * MB
    return (rs.uniform(0.0, 1.0, (n, NCLS)).astype(np.float32),
            (rs.uniform(0.0, 1.0, (n, NCLS)) < 0.35).astype(np.float32))


def rank_batches(world, rank):
    """The (first row, last row) of the batches rank `rank` sees, in its order."""
    return [((i * world + rank) * MB, (i * world + rank + 1) * MB) for i in range(MAX_ITER)]


class _Cfg(object):
    def __init__(self, world):
        self.LOG_PERIOD, self.NUM_GPUS = 2, world
        self.SOLVER = type("S", (), {"MAX_EPOCH": 1})()
        self.DATA = type("D", (), {"MULTI_LABEL": True})()
        self.TRAIN = type("T", (), {"TOPK": 5})()


def main():
    out_dir = sys.argv[1]
    backend = sys.argv[2] if len(sys.argv) > 2 else "nccl"
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(int(sys.argv[3]) if len(sys.argv) > 3 else rank)
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank,
                            world_size=world)
    try:
        from slowfast.utils.meters import DeviceValMeter
        from _host_reads import count_host_reads as _count_host_reads
        preds, labels = epoch_rows(world)
        m = DeviceValMeter(MAX_ITER, _Cfg(world))
        with _count_host_reads() as seen:
            for i, (lo, hi) in enumerate(rank_batches(world, rank)):
                m.update_predictions(torch.from_numpy(preds[lo:hi]).cuda(), torch.from_numpy(labels[lo:hi]).cuda())
                m.log_iter_stats(0, i)
            stats = m.log_epoch_stats(0)
        with open(os.path.join(out_dir, "valmap_rank%d.json" % rank), "w") as f:
            json.dump({"map": stats["map"], "host_reads": len(seen), "cap": m.cap, "rows": m._appended}, f)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
