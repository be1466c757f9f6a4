"""Counting the calls that bring a GPU tensor to the host (tests/test_eval_metrics_gpu.py, tests/_val_map_worker.py)."""
import contextlib

import torch


@contextlib.contextmanager
def count_host_reads():
    """Counts the calls that copy a GPU tensor to the host (tools/count_torch_ops.py's method: wrap the tensor methods
    and count the ones made on a device tensor, `copy_` into a host tensor included)."""
    seen = []
    names = ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__", "__index__")
    orig = {n: getattr(torch.Tensor, n) for n in names + ("to", "copy_")}

    def wrap(name):
        def f(t, *a, **k):
            if t.is_cuda:
                seen.append(name)
            return orig[name](t, *a, **k)
        return f

    def to(t, *a, **k):
        dst = k.get("device", a[0] if a else None)
        if t.is_cuda and (dst == "cpu" or (isinstance(dst, torch.device) and dst.type == "cpu")):
            seen.append("to")
        return orig["to"](t, *a, **k)

    def copy_(t, src, *a, **k):
        if isinstance(src, torch.Tensor) and src.is_cuda and not t.is_cuda:
            seen.append("copy_")
        return orig["copy_"](t, src, *a, **k)
    for n in names:
        setattr(torch.Tensor, n, wrap(n))
    torch.Tensor.to = to
    torch.Tensor.copy_ = copy_
    try:
        yield seen
    finally:
        for n, f in orig.items():
            setattr(torch.Tensor, n, f)
