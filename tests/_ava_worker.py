"""One rank of the two-rank detection evaluation (tests/test_ava_eval_gpu.py): RANK / WORLD_SIZE / MASTER_PORT from the
environment as tests/_val_map_worker.py takes them.  Every rank hands ITS OWN contiguous, unevenly sized share of the
seeded epoch's rows to a DeviceAVAMeter with NUM_GPUS = world in uneven batches, finalizes, and leaves {"map", "rows",
"host_reads"} in <out_dir>/ava_rank<r>.json.

usage: _ava_worker.py <out_dir> [backend [device]]   (default: nccl on device RANK)"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

K = 257


def epoch_case(world):
    import _ava_cases
    return _ava_cases.random_case(K)


def rank_rows(world, rank):
    """(first row, last row) of rank `rank`: shares of different sizes, in rank order."""
    cuts = [0] + [K * (r + 1) // world + (7 if r + 1 < world else 0) for r in range(world)]
    return cuts[rank], cuts[rank + 1]


def main():
    out_dir = sys.argv[1]
    backend = sys.argv[2] if len(sys.argv) > 2 else "nccl"
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(int(sys.argv[3]) if len(sys.argv) > 3 else rank)
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:%s" % os.environ["MASTER_PORT"], rank=rank,
                            world_size=world)
    try:
        from slowfast.utils.meters import DeviceAVAMeter
        from _host_reads import count_host_reads
        from _ava_cases import MeterCfg, write_case_files
        case = epoch_case(world)
        d = tempfile.mkdtemp()
        write_case_files(case, d)
        m = DeviceAVAMeter(4, MeterCfg(d, True, num_gpus=world), "val", video_idx_to_name=case["names"])
        lo, hi = rank_rows(world, rank)
        dev = [torch.from_numpy(case[k][lo:hi]).cuda() for k in ("preds", "boxes", "metadata")]
        with count_host_reads() as seen:
            for a in range(0, hi - lo, 50):
                m.update_stats(*(t[a:a + 50] for t in dev))
            value = m.finalize_metrics(log=False)
        with open(os.path.join(out_dir, "ava_rank%d.json" % rank), "w") as f:
            json.dump({"map": value, "rows": m.rows, "host_reads": len(seen)}, f)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
