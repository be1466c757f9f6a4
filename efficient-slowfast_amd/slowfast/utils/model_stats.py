"""Watching a run on libsfhip kernels (csrc/tensor_stats.hip): what the reference's TensorboardWriter
(visualization/tensorboard_vis.py, TENSORBOARD.MODEL_VIS) is there for — which layer went dead, which gradient vanished,
where the first Inf appeared — as ONE native call per recording over an address table of every parameter or gradient.

* `DeviceModelStats(named_tensors, slots=8)` — `record("param" | "grad")` is one `sf_tensor_stats` call (two launches, every
  element read once, no host read, capturable) that writes the statistics row of every tensor into the next slot of a
  ring in device memory; `read()` is one device-to-host copy of that ring, once per logging period.
* `TensorStats` — a tensor's row with `mean`, `rms`, `std` derived on the host; `to_scalars` / `to_histogram_raw` turn
  rows into what `TensorboardWriter.add_scalars` / `SummaryWriter.add_histogram_raw` take (nothing here imports
  tensorboard); `first_bad` names the first tensor with a NaN or an Inf.
* `construct_model_stats(cfg, model)` — TENSORBOARD.ENABLE and TENSORBOARD.MODEL_VIS.ENABLE.
There is no fallback: tensors that are not contiguous float32 tensors on the current GPU are refused."""
import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch

import sfhip

BINS = sfhip.SF_TSTATS_BINS            # exponent bins per sign
ROW = sfhip.SF_TSTATS_ROW              # 8-byte slots of a tensor's row
N_HIST = 2 * BINS + 1
EXP_LO = -20                           # |x| < 2^EXP_LO: the centre bin
COL_PRESENT, COL_NUMEL, COL_NAN, COL_INF, COL_ZERO, COL_MINMAX, COL_ABSMAX, COL_SUM, COL_SUMSQ, COL_HIST = range(10)
# the bins' upper limits, increasing: the negative side from the largest magnitude down, the centre bin, the positive side
# (the outermost bins are open: -2^3 closes the first, 2^4 is the nominal end of the last)
BUCKET_LIMITS = tuple([-(2.0 ** e) for e in range(EXP_LO + BINS - 1, EXP_LO - 1, -1)] + [2.0 ** EXP_LO] +
                      [2.0 ** e for e in range(EXP_LO + 1, EXP_LO + BINS + 1)])

TensorStats = namedtuple("TensorStats", ["present", "numel", "n_nan", "n_inf", "n_zero", "min", "max", "absmax", "sum",
                                         "sumsq", "hist", "n_finite", "mean", "rms", "std"])


def parse_rows(rows):
    """rows: int64 numpy [n, ROW] as the kernel wrote them -> [TensorStats] (hist: a tuple of 2 * BINS + 1 ints).  mean,
    rms and std (the population's) are over the finite elements and NaN when there are none."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    f32, f64 = rows.view(np.float32), rows.view(np.float64)
    out = []
    for i in range(rows.shape[0]):
        r = rows[i]
        numel, n_nan, n_inf = int(r[COL_NUMEL]), int(r[COL_NAN]), int(r[COL_INF])
        s, ss = float(f64[i, COL_SUM]), float(f64[i, COL_SUMSQ])
        n = numel - n_nan - n_inf
        if n > 0:
            mean = s / n
            rms = math.sqrt(ss / n)
            std = math.sqrt(max(ss / n - mean * mean, 0.0))
        else:
            mean = rms = std = float("nan")
        out.append(TensorStats(int(r[COL_PRESENT]), numel, n_nan, n_inf, int(r[COL_ZERO]),
                               float(f32[i, 2 * COL_MINMAX]), float(f32[i, 2 * COL_MINMAX + 1]),
                               float(f32[i, 2 * COL_ABSMAX]), s, ss, tuple(int(v) for v in r[COL_HIST:COL_HIST + N_HIST]),
                               n, mean, rms, std))
    return out


class _AddressTable(object):
    """The (address, numel) table of one recording kind in host and device memory; the chunk list depends on the numels
    only and is shared."""

    def __init__(self):
        self.sig = None
        self.host = self.dev = None
        self.rebuilds = 0


class DeviceModelStats(object):
    """Per-tensor statistics and sign-and-exponent histograms of a model's parameters and gradients:

        watch = DeviceModelStats(model.named_parameters())
        loss.backward(); watch.record("grad"); optimizer.step(); watch.record("param")     # one native call each
        if step % period == 0:
            for stats in watch.read("grad"): writer.add_scalars(to_scalars(stats, "grad"), step)

    `named_tensors`: (name, tensor) pairs, contiguous float32 tensors on the current GPU (empty ones have no row).
    `record(which)` writes the row of every tensor — `which="grad"`: of its `.grad`; a `.grad` that is None gives the
    all-zero row with present = 0 — into the next of `slots` ring slots and advances the device-side cursor: no host
    read, no allocation, so it can run every step and inside a captured graph.  The address tables are built once and
    rebuilt only when an ADDRESS changes (`rebuilds[which]` counts: the training tape's flat gradient buffer keeps the
    addresses, so a second step reuses the table); a rebuild takes a host-to-device copy and is refused under stream
    capture — warm up eagerly first.  Each kind has a workspace, a ring and a cursor of its own (ring and cursor in one
    allocation, so `read(which)` is ONE device-to-host copy); the recordings of ONE kind must follow each other on one
    stream, as must a `read` and the recordings it reports.  `read` returns the recorded slots, oldest first, each an
    OrderedDict name -> TensorStats in table order."""

    def __init__(self, named_tensors, slots=8):
        named = [(n, t) for n, t in named_tensors]
        if int(slots) <= 0:
            raise ValueError("DeviceModelStats: slots must be positive, got %r" % (slots,))
        self.slots = int(slots)
        seen = set()
        for name, t in named:
            if not torch.is_tensor(t):
                raise ValueError("DeviceModelStats: %r is a %s, not a tensor" % (name, type(t).__name__))
            if name in seen:
                raise ValueError("DeviceModelStats: duplicate name %r" % (name,))
            seen.add(name)
            if t.dtype != torch.float32:
                raise ValueError("DeviceModelStats: %r has dtype %s — float32 only" % (name, t.dtype))
            if not t.is_contiguous():
                raise ValueError("DeviceModelStats: %r is not contiguous" % (name,))
        named = [(n, t) for n, t in named if t.numel() > 0]
        if not named:
            raise ValueError("DeviceModelStats: no tensor to watch")
        for name, t in named:
            sfhip._require_gpu(t, "DeviceModelStats(%s)" % name)
        from slowfast.models.step_tail import build_clip_tables  # the (address, numel) table the clipper uses
        self.names = [n for n, _ in named]
        self._tensors = [t for _, t in named]
        self.device = self._tensors[0].device
        n = len(named)
        table, self._chunks = build_clip_tables([(0, t.numel()) for t in self._tensors],
                                                sfhip.lib().sf_sgd_chunk_elems())
        self._chunks_dev = self._chunks.to(self.device)
        self._numels = table[:, 1].clone()
        ws_bytes = sfhip.lib().sf_tensor_stats_ws_bytes(self._chunks.shape[0])
        self._tabs = {"param": _AddressTable(), "grad": _AddressTable()}
        # a workspace per kind: the two recordings share nothing, so they may run on different streams
        self._ws = {k: torch.empty(((ws_bytes + 7) // 8,), dtype=torch.int64, device=self.device) for k in self._tabs}
        # per kind: [slots * n * ROW] ring words, then ONE word = the int32 pair {next slot, calls made}
        self._store = {k: torch.zeros((self.slots * n * ROW + 1,), dtype=torch.int64, device=self.device)
                       for k in self._tabs}
        self.rebuilds = {"param": 0, "grad": 0}

    def ring(self, which):
        """The ring of one kind: an int64 [slots, n_tensors, ROW] view in device memory."""
        return self._store[which][:-1].view(self.slots, len(self.names), ROW)

    def cursor(self, which):
        """Its cursor: an int32 [2] view in device memory = next slot, calls made."""
        return self._store[which][-1:].view(torch.int32)

    def _addresses(self, which):
        if which == "param":
            return [t.data_ptr() for t in self._tensors]
        out = []
        for name, t in zip(self.names, self._tensors):
            g = t.grad
            if g is None:
                out.append(0)
                continue
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != t.numel():
                raise ValueError("DeviceModelStats: the gradient of %r must be a contiguous float32 tensor of the "
                                 "parameter's size" % (name,))
            sfhip._require_gpu(g, "DeviceModelStats(%s.grad)" % name)
            out.append(g.data_ptr())
        return out

    @torch.no_grad()
    def record(self, which="param"):
        """One `sf_tensor_stats` call over every tensor (`which="param"`) or every `.grad` (`which="grad"`)."""
        if which not in self._tabs:
            raise ValueError("DeviceModelStats.record: which is 'param' or 'grad', got %r" % (which,))
        tab = self._tabs[which]
        sig = self._addresses(which)
        if sig != tab.sig:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceModelStats.record under stream capture needs a new address table, which takes a "
                                   "host-to-device copy — warm up eagerly first (record once outside the capture)")
            tab.host = torch.stack([torch.tensor(sig, dtype=torch.int64), self._numels], dim=1).contiguous()
            if tab.dev is None:
                tab.dev = tab.host.to(self.device)
            else:
                tab.dev.copy_(tab.host)
            tab.sig = sig
            self.rebuilds[which] += 1
        sfhip.tensor_stats(tab.host, tab.dev, self._chunks, self._chunks_dev, self._ws[which], self.ring(which),
                           self.cursor(which))

    def read(self, which="param"):
        """ONE device-to-host copy of the ring of `which` -> the recorded slots, oldest first (at most `slots`), each an
        OrderedDict name -> TensorStats in table order."""
        if which not in self._tabs:
            raise ValueError("DeviceModelStats.read: which is 'param' or 'grad', got %r" % (which,))
        host = self._store[which].cpu().numpy()
        nxt, made = (int(v) for v in host[-1:].view(np.int32))
        rows = host[:-1].reshape(self.slots, len(self.names), ROW)
        have = min(max(made, 0), self.slots)
        out = []
        for i in range(have):
            slot = (nxt - have + i) % self.slots
            out.append(OrderedDict(zip(self.names, parse_rows(rows[slot]))))
        return out


def first_bad(stats):
    """The name of the first tensor, in table order, with a NaN or an Inf (what to look at after the guard tripped), or
    None."""
    for name, ts in stats.items():
        if ts.n_nan + ts.n_inf > 0:
            return name
    return None


def to_scalars(stats, prefix):
    """The flat {tag: value} dict `TensorboardWriter.add_scalars` takes: per present tensor `<prefix>/<name>/rms`,
    `/absmax`, `/zero_frac`, `/nonfinite`, and the same over all of them under `<prefix>/global/` with `/norm` (the L2
    norm of the finite elements)."""
    out = OrderedDict()
    numel = n_fin = n_zero = n_bad = 0
    sumsq, absmax = 0.0, 0.0
    for name, ts in stats.items():
        if not ts.present:
            continue
        out["%s/%s/rms" % (prefix, name)] = ts.rms
        out["%s/%s/absmax" % (prefix, name)] = ts.absmax
        out["%s/%s/zero_frac" % (prefix, name)] = ts.n_zero / ts.numel
        out["%s/%s/nonfinite" % (prefix, name)] = ts.n_nan + ts.n_inf
        numel += ts.numel
        n_fin += ts.n_finite
        n_zero += ts.n_zero
        n_bad += ts.n_nan + ts.n_inf
        sumsq += ts.sumsq
        absmax = max(absmax, ts.absmax)
    out["%s/global/rms" % prefix] = math.sqrt(sumsq / n_fin) if n_fin > 0 else float("nan")
    out["%s/global/norm" % prefix] = math.sqrt(sumsq)
    out["%s/global/absmax" % prefix] = absmax
    out["%s/global/zero_frac" % prefix] = n_zero / numel if numel > 0 else 0.0
    out["%s/global/nonfinite" % prefix] = n_bad
    return out


def to_histogram_raw(ts):
    """The keyword arguments of `SummaryWriter.add_histogram_raw` for one TensorStats: the finite elements' min, max,
    count, sum and sum of squares, the 2 * BINS + 1 increasing bucket limits and the bucket counts.  The kernel's bins are
    [2^e, 2^(e+1)) in magnitude while tensorboard reads a bucket as (limit[i - 1], limit[i]]: on the negative side the two
    agree, on the positive side a value that is exactly a power of two (+2^-20 itself included) is counted in the bucket
    ABOVE the limit it equals.  The outermost buckets are open: everything at or beyond +-2^3 is in them."""
    return {"min": ts.min if ts.n_finite > 0 else 0.0, "max": ts.max if ts.n_finite > 0 else 0.0, "num": ts.n_finite,
            "sum": ts.sum, "sum_squares": ts.sumsq, "bucket_limits": list(BUCKET_LIMITS),
            "bucket_counts": list(ts.hist)}


def construct_model_stats(cfg, model, slots=8):
    """TENSORBOARD.ENABLE and TENSORBOARD.MODEL_VIS.ENABLE -> a DeviceModelStats over `model.named_parameters()`, else
    None."""
    if not (cfg.TENSORBOARD.ENABLE and cfg.TENSORBOARD.MODEL_VIS.ENABLE):
        return None
    return DeviceModelStats(model.named_parameters(), slots=slots)
