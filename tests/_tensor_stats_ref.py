"""The statistics row of sf_tensor_stats (include/sfhip.h) restated in numpy from its definition, not from any
implementation: integer fields exact, the bin of a finite element from np.frexp, the fp64 sums with math.fsum (correctly
rounded, so the reference's own error is half an ulp)."""
import math
from collections import namedtuple

import numpy as np

B = 24                 # exponent bins per sign
N_HIST = 2 * B + 1
EXP_LO = -20           # |x| < 2^EXP_LO: the centre bin

Row = namedtuple("Row", ["present", "numel", "n_nan", "n_inf", "n_zero", "min", "max", "absmax", "sum", "sumsq", "hist",
                         "sum_abs", "sumsq_abs"])


def bin_of(x):
    """The histogram bin of ONE finite float32 value: frexp gives |x| = m * 2^p with 0.5 <= m < 1, so
    floor(log2 |x|) = p - 1 (denormals included: frexp normalises them)."""
    x = np.float32(x)
    assert np.isfinite(x)
    a = abs(float(x))
    if a < 2.0 ** EXP_LO:
        return B
    e = int(np.frexp(np.float64(a))[1]) - 1
    k = min(max(e - EXP_LO, 0), B - 1)
    return B + 1 + k if x > 0 else B - 1 - k


def ref_row(x):
    """x: a float32 numpy array (any shape) -> Row.  sum_abs / sumsq_abs: the sums of |term|, for the accumulation
    bound."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    nan, inf = np.isnan(x), np.isinf(x)
    fin = x[~(nan | inf)]
    hist = [0] * N_HIST
    if fin.size:
        a = np.abs(fin.astype(np.float64))
        e = np.frexp(a)[1].astype(np.int64) - 1
        k = np.clip(e - EXP_LO, 0, B - 1)
        idx = np.where(a < 2.0 ** EXP_LO, B, np.where(fin > 0, B + 1 + k, B - 1 - k))
        hist = np.bincount(idx, minlength=N_HIST).tolist()
    wide = [float(v) for v in fin.astype(np.float64)]
    return Row(1, int(x.size), int(nan.sum()), int(inf.sum()), int((x == 0).sum()),
               np.float32(fin.min()) if fin.size else np.float32(np.inf),
               np.float32(fin.max()) if fin.size else np.float32(-np.inf),
               np.float32(np.abs(fin).max()) if fin.size else np.float32(0.0),
               math.fsum(wide), math.fsum(v * v for v in wide), tuple(int(h) for h in hist),
               math.fsum(abs(v) for v in wide), math.fsum(v * v for v in wide))


ABSENT = Row(0, 0, 0, 0, 0, np.float32(0.0), np.float32(0.0), np.float32(0.0), 0.0, 0.0, (0,) * N_HIST, 0.0, 0.0)


def edge_values():
    """Every bin-edge value the tests plant: +-2^-20 with the floats just below and above, 2^3, 2^4, FLT_MAX, the
    smallest normal, a denormal, +-0."""
    f = np.float32
    lo = f(2.0 ** EXP_LO)
    out = []
    for s in (f(1.0), f(-1.0)):
        out += [s * lo, s * np.nextafter(lo, f(0.0)), s * np.nextafter(lo, f(1.0))]
    out += [f(8.0), f(16.0), np.finfo(np.float32).max, np.finfo(np.float32).tiny, f(1e-40), f(0.0), f(-0.0)]
    return np.array(out, dtype=np.float32)


def check_row(got, ref, tag=""):
    """got: a slowfast.utils.model_stats.TensorStats; ref: a Row.  Integer fields and min / max / absmax exactly; sum and
    sumsq within numel * 2^-52 * sum |term| (the fp64 accumulation bound: each of the numel - 1 additions rounds by at
    most 2^-53 of a partial sum that never exceeds sum |term|)."""
    for f in ("present", "numel", "n_nan", "n_inf", "n_zero", "hist"):
        assert getattr(got, f) == getattr(ref, f), (tag, f, getattr(got, f), getattr(ref, f))
    for f in ("min", "max", "absmax"):
        assert np.float32(getattr(got, f)) == getattr(ref, f), (tag, f, getattr(got, f), getattr(ref, f))
    assert sum(got.hist) + got.n_nan + got.n_inf == got.numel, tag
    for f, bound in (("sum", ref.sum_abs), ("sumsq", ref.sumsq_abs)):
        err, tol = abs(getattr(got, f) - getattr(ref, f)), ref.numel * 2.0 ** -52 * bound
        assert err <= tol, (tag, f, getattr(got, f), getattr(ref, f), err, tol)
