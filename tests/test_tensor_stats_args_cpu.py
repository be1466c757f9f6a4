"""Host side of the training telemetry (sf_tensor_stats, sf_tensor_stats_ws_bytes, slowfast/utils/model_stats.py): the
exports, the audit's hot list, every refusal of the entry point (checked before any launch, so callable without a
GPU), the Python layer's refusals, and the host-side helpers (parse_rows, to_scalars, to_histogram_raw, first_bad,
construct_model_stats) on rows made by the reference."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import _tensor_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _good():
    from slowfast.models.step_tail import build_clip_tables
    C = _chunk()
    entries, addr = [], FAKE
    for n in (C, 1, 3, 4, 5, C - 1, C + 1, 2 * C + 1):
        entries.append((addr, n))
        addr += 4 * n
    return build_clip_tables(entries, C)


def _rc(table, chunks, null=None, put=None):
    """sf_tensor_stats with fake device addresses; `null`: positions handed None, `put`: {position: value}."""
    import sfhip
    L = sfhip.lib()
    dev = ctypes.c_void_p(FAKE)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], dev,
            L.sf_tensor_stats_ws_bytes(chunks.shape[0]), dev, sfhip.SF_TSTATS_ROW, 3,
            ctypes.cast(dev, sfhip._pi), None]
    if null is not None:
        args[null] = None
    for k, v in (put or {}).items():
        args[k] = v
    return L.sf_tensor_stats(*args)


def test_symbols_constants_and_the_hot_list():
    import sfhip
    assert "sf_tensor_stats" in sfhip.EXPORTS and "sf_tensor_stats_ws_bytes" in sfhip.EXPORTS
    txt = open(os.path.join(ROOT, "include", "sfhip.h")).read()
    assert "#define SF_TSTATS_ROW %d\n" % sfhip.SF_TSTATS_ROW in txt
    assert "#define SF_TSTATS_BINS %d\n" % sfhip.SF_TSTATS_BINS in txt
    assert sfhip.SF_TSTATS_BINS == ref.B and sfhip.SF_TSTATS_ROW == 9 + ref.N_HIST
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    assert "tstats_partial_kernel" in audit.HOT and "tstats_finish_kernel" in audit.HOT
    assert not any(e.startswith("tstats_") for e in audit.EXEMPT)


def test_workspace_size_query_is_host_only():
    import sfhip
    L = sfhip.lib()
    assert L.sf_tensor_stats_ws_bytes(0) == 0 and L.sf_tensor_stats_ws_bytes(-3) == 0
    one, two = L.sf_tensor_stats_ws_bytes(1), L.sf_tensor_stats_ws_bytes(2)
    assert 0 < one < two and one % 8 == 0 and two % 8 == 0
    per = two - one  # a chunk's row: two fp64 sums, min / max, 52 int32 counts — and the tensor's first-chunk word
    assert per >= 16 + 8 + 4 * (ref.N_HIST + 3)
    assert L.sf_tensor_stats_ws_bytes(1000) == one + 999 * per


def test_refusals():
    import sfhip
    table, chunks = _good()
    E, A = sfhip.SF_EINVAL, sfhip.SF_EALIGN
    for null in (0, 1, 3, 4, 6, 8, 11):  # table_host, table, chunks_host, chunks, ws, ring, cursor
        assert _rc(table, chunks, null=null) == E, null
    for pos in (2, 5):  # n_tensors, n_chunks
        for v in (0, -1):
            assert _rc(table, chunks, put={pos: v}) == E, (pos, v)
    for row in (sfhip.SF_TSTATS_ROW - 1, sfhip.SF_TSTATS_ROW + 1, 0, 8):  # the caller's row width is not the library's
        assert _rc(table, chunks, put={9: row}) == E, row
    for slots in (0, -1):
        assert _rc(table, chunks, put={10: slots}) == E, slots
    need = sfhip.lib().sf_tensor_stats_ws_bytes(chunks.shape[0])
    for b in (need - 1, need - 8, 0, -1):  # a workspace that is too small
        assert _rc(table, chunks, put={7: b}) == E, b

    def bad_row(col, value, row=4):
        t = table.clone()
        t[row, col] = value
        return _rc(t, chunks)
    assert bad_row(0, FAKE + 2) == E and bad_row(0, FAKE + 1) == E      # an address off 4 bytes
    assert bad_row(1, 0) == E and bad_row(1, -5) == E                    # numel <= 0
    C = _chunk()
    for c in (chunks[:-1], torch.cat([chunks, chunks[-1:]]), chunks.flip(0), torch.cat([chunks[:1], chunks]),
              torch.where(chunks == C, torch.tensor(C - 4), chunks),
              torch.cat([chunks[:5], torch.tensor([[4, C]]), chunks[5:]])):
        assert _rc(table, c.contiguous()) == E
    t = table.clone()
    t[6, 1] = C  # a numel the chunk list does not tile
    assert _rc(t, chunks) == E
    dev = lambda a: ctypes.c_void_p(a)
    assert _rc(table, chunks, put={6: dev(FAKE + 4)}) == A and _rc(table, chunks, put={8: dev(FAKE + 4)}) == A
    assert _rc(table, chunks, put={11: ctypes.cast(dev(FAKE + 2), sfhip._pi)}) == A


def test_python_layer_refusals():
    import sfhip
    from slowfast.utils.model_stats import DeviceModelStats
    ok = torch.zeros(4, 3)
    with pytest.raises(sfhip.SfhipError, match="GPU"):
        DeviceModelStats([("w", ok)])                                    # a CPU tensor
    with pytest.raises(ValueError, match="float32"):
        DeviceModelStats([("w", ok.double())])
    with pytest.raises(ValueError, match="float32"):
        DeviceModelStats([("w", ok), ("h", ok.half())])
    with pytest.raises(ValueError, match="contiguous"):
        DeviceModelStats([("w", ok.t())])
    with pytest.raises(ValueError, match="duplicate"):
        DeviceModelStats([("w", ok), ("b", ok.clone()), ("w", ok.clone())])
    with pytest.raises(ValueError, match="slots"):
        DeviceModelStats([("w", ok)], slots=0)
    with pytest.raises(ValueError, match="no tensor"):
        DeviceModelStats([])
    with pytest.raises(ValueError, match="tensor"):
        DeviceModelStats([("w", 3.0)])


def _rows_of(arrays):
    """The kernel's int64 rows for a list of float32 arrays (None: absent), written from the reference."""
    import sfhip
    from slowfast.utils import model_stats as ms
    rows = np.zeros((len(arrays), sfhip.SF_TSTATS_ROW), dtype=np.int64)
    f32, f64 = rows.view(np.float32), rows.view(np.float64)
    for i, a in enumerate(arrays):
        if a is None:
            continue
        r = ref.ref_row(a)
        rows[i, :5] = (1, r.numel, r.n_nan, r.n_inf, r.n_zero)
        f32[i, 2 * ms.COL_MINMAX], f32[i, 2 * ms.COL_MINMAX + 1], f32[i, 2 * ms.COL_ABSMAX] = r.min, r.max, r.absmax
        f64[i, ms.COL_SUM], f64[i, ms.COL_SUMSQ] = r.sum, r.sumsq
        rows[i, ms.COL_HIST:] = r.hist
    return rows


def test_host_helpers_on_reference_rows():
    from collections import OrderedDict
    from slowfast.utils import model_stats as ms
    a = np.array([1.0, -3.0, 0.0, 0.5], dtype=np.float32)
    b = np.array([2.0, np.nan, np.inf, -4.0, 0.0, 0.0], dtype=np.float32)
    stats = OrderedDict(zip(["a", "gone", "b", "c"], ms.parse_rows(_rows_of([a, None, b, a * 2]))))
    ta, tb = stats["a"], stats["b"]
    assert (ta.present, ta.numel, ta.n_zero, ta.n_finite, ta.min, ta.max, ta.absmax) == (1, 4, 1, 4, -3.0, 1.0, 3.0)
    assert ta.mean == -1.5 / 4 and ta.rms == math.sqrt(10.25 / 4)
    assert abs(ta.std - float(np.std(a.astype(np.float64)))) < 1e-15
    assert (tb.n_nan, tb.n_inf, tb.n_finite, tb.sum, tb.sumsq) == (1, 1, 4, -2.0, 20.0)
    assert stats["gone"].present == 0 and math.isnan(stats["gone"].rms) and sum(stats["gone"].hist) == 0
    assert ms.first_bad(stats) == "b"
    assert ms.first_bad(OrderedDict([("a", ta), ("c", stats["c"])])) is None

    sc = ms.to_scalars(stats, "grad")
    assert not any(k.startswith("grad/gone/") for k in sc)  # an absent tensor has no scalars
    assert sc["grad/a/rms"] == ta.rms and sc["grad/a/absmax"] == 3.0 and sc["grad/a/zero_frac"] == 0.25
    assert sc["grad/b/nonfinite"] == 2 and sc["grad/b/zero_frac"] == 2 / 6
    assert sc["grad/global/nonfinite"] == 2 and sc["grad/global/absmax"] == 6.0
    assert sc["grad/global/zero_frac"] == 4 / 14
    tot = 10.25 + 20.0 + 41.0
    assert sc["grad/global/norm"] == math.sqrt(tot) and sc["grad/global/rms"] == math.sqrt(tot / 12)
    assert all(isinstance(k, str) and isinstance(v, (int, float)) for k, v in sc.items())


def test_histogram_raw_needs_no_tensorboard():
    from slowfast.utils import model_stats as ms
    b = np.array([2.0, np.nan, np.inf, -4.0, 0.0, 0.0, 2.0 ** -20, -20.0, 1e-40], dtype=np.float32)
    loaded = {m for m in sys.modules if "tensorboard" in m}
    ts = ms.parse_rows(_rows_of([b]))[0]
    kw = ms.to_histogram_raw(ts)
    assert {m for m in sys.modules if "tensorboard" in m} == loaded      # the call imported none of it
    assert not re.search(r"^\s*(import|from)\s+\S*tensorboard", open(ms.__file__).read(), re.M | re.I)
    assert sorted(kw) == ["bucket_counts", "bucket_limits", "max", "min", "num", "sum", "sum_squares"]
    lim, cnt = kw["bucket_limits"], kw["bucket_counts"]
    assert len(lim) == len(cnt) == 2 * ref.B + 1
    assert all(x < y for x, y in zip(lim, lim[1:]))                       # strictly increasing
    assert lim[0] == -8.0 and lim[ref.B - 1] == -2.0 ** -20 and lim[ref.B] == 2.0 ** -20 and lim[-1] == 16.0
    assert kw["num"] == sum(cnt) == 7 and kw["min"] == -20.0 and kw["max"] == 2.0
    assert kw["sum"] == ts.sum and kw["sum_squares"] == ts.sumsq
    # every finite element sits under its bucket's upper limit and, past the first bucket, at or above the one before
    # (up to the side of the limit itself: the kernel's bins are closed towards zero's far side, [2^e, 2^(e+1)))
    for v in b[np.isfinite(b)]:
        i = ref.bin_of(v)
        assert (i == len(lim) - 1 or v <= lim[i]) and (i == 0 or v >= lim[i - 1]), (v, i)
    empty = ms.to_histogram_raw(ms.parse_rows(_rows_of([np.array([np.nan], dtype=np.float32)]))[0])
    assert (empty["min"], empty["max"], empty["num"]) == (0.0, 0.0, 0)


def test_construct_model_stats_reads_the_config():
    from slowfast.config.defaults import get_cfg
    from slowfast.utils.model_stats import construct_model_stats
    import sfhip
    cfg = get_cfg()
    model = torch.nn.Linear(3, 2)
    assert cfg.TENSORBOARD.MODEL_VIS.ENABLE is False       # the reference's default
    assert construct_model_stats(cfg, model) is None
    cfg.TENSORBOARD.MODEL_VIS.ENABLE = True
    cfg.TENSORBOARD.ENABLE = False
    assert construct_model_stats(cfg, model) is None
    cfg.TENSORBOARD.ENABLE = True
    with pytest.raises(sfhip.SfhipError):                  # a CPU model: there is no fallback
        construct_model_stats(cfg, model)
