"""Host side of gradient clipping (csrc/grad_clip.hip, slowfast/models/step_tail.py::HipGradClip, DeviceTrainMeter's
grad_norm window): the (gradient address, numel) table and its chunk tiling, every refusal of sf_grad_norm /
sf_grad_scale / sf_grad_clamp (checked on the host copies before any launch, so callable without a GPU), every
refusal of HipGradClip, construct_hip_grad_clip, and the meter's drain of column 7 on a CPU ring."""
import ctypes
import math

import numpy as np
import pytest
import torch

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _numels():
    C = _chunk()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1]


def _entries(numels):
    out, addr = [], FAKE
    for n in numels:
        out.append((addr, n))
        addr += 4 * n
    return out


def test_table_builder_rows_and_chunk_tiling():
    from slowfast.models.step_tail import build_clip_tables
    C = _chunk()
    numels = _numels()
    entries = _entries(numels)
    table, chunks = build_clip_tables(entries, C)
    assert table.dtype == torch.int64 and chunks.dtype == torch.int64 and tuple(table.shape) == (len(numels), 2)
    assert table.tolist() == [list(e) for e in entries]
    want = []
    for i, n in enumerate(numels):
        want += [[i, s] for s in range(0, n, C)]
    assert chunks.tolist() == want
    # C - 1 and C: one chunk; C + 1: two; 2C + 1: three — no chunk straddles a tensor, none is empty
    assert [sum(1 for c in want if c[0] == i) for i in range(len(numels))] == [1, 1, 1, 1, 1, 1, 2, 3]
    for i, s in want:
        assert 0 <= s < numels[i] and s % C == 0


def _tables():
    from slowfast.models.step_tail import build_clip_tables
    return build_clip_tables(_entries(_numels()), _chunk())


def _rc(symbol, table, chunks, null=None, counts=None, tail=None):
    """`symbol` on host tables and FAKE device addresses; tail: the arguments behind n_chunks, stream excluded."""
    import sfhip
    L = sfhip.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = ctypes.c_void_p(FAKE)
    args = [vp(table), dev, table.shape[0], vp(chunks), dev, chunks.shape[0]]
    if tail is None:
        tail = _norm_tail() if symbol == "sf_grad_norm" else [dev]
    args += list(tail) + [None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return getattr(L, symbol)(*args)


def _norm_tail(norm_type=2, partials=FAKE, state=FAKE, ring=None, counter=None, cap=0):
    import sfhip
    p = lambda a: ctypes.c_void_p(a) if a is not None else None
    cnt = ctypes.cast(ctypes.c_void_p(counter), sfhip._pi) if counter is not None else None
    return [norm_type, p(FAKE), None, p(partials), p(state), p(ring), cnt, cap]


@pytest.mark.parametrize("symbol", ["sf_grad_norm", "sf_grad_scale", "sf_grad_clamp"])
def test_table_refusals_of_every_entry(symbol):
    import sfhip
    table, chunks = _tables()
    E = sfhip.SF_EINVAL
    for null in (0, 1, 3, 4):
        assert _rc(symbol, table, chunks, null=null) == E, null
    for pos in (2, 5):  # n_tensors, n_chunks
        for v in (0, -1):
            assert _rc(symbol, table, chunks, counts={pos: v}) == E, (pos, v)

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _rc(symbol, t, chunks)
    assert bad_row(0, 0) == E                                              # null gradient address
    assert bad_row(0, FAKE + 2) == E and bad_row(0, FAKE + 1) == E         # not even a float's alignment
    assert bad_row(1, 0) == E and bad_row(1, -5) == E                      # numel <= 0
    C = _chunk()
    for mutate in (lambda c: c[:-1], lambda c: torch.cat([c, c[-1:]]), lambda c: c.flip(0),
                   lambda c: torch.cat([c[:1], c]),
                   lambda c: torch.where(c == C, torch.tensor(C - 4), c),           # a start off the chunk grid
                   lambda c: torch.cat([c[:5], torch.tensor([[4, C]]), c[5:]])):    # a chunk past its tensor's end
        assert _rc(symbol, table, mutate(chunks.clone()).contiguous()) == E


def test_grad_norm_own_refusals():
    import sfhip
    table, chunks = _tables()
    E, A = sfhip.SF_EINVAL, sfhip.SF_EALIGN
    rc = lambda **kw: _rc("sf_grad_norm", table, chunks, tail=_norm_tail(**kw))
    for nt in (1, 3, -1, 4):
        assert rc(norm_type=nt) == E, nt
    assert rc(partials=None) == E and rc(state=None) == E
    assert rc(partials=FAKE + 4) == A and rc(state=FAKE + 4) == A          # an fp64 lives in both
    assert rc(ring=FAKE, counter=None, cap=4) == E and rc(ring=None, counter=FAKE, cap=4) == E
    assert rc(ring=FAKE, counter=FAKE, cap=0) == E and rc(ring=FAKE, counter=FAKE, cap=-2) == E
    # scale: a null or misaligned state; clamp: a null value
    assert _rc("sf_grad_scale", table, chunks, tail=[None]) == E
    assert _rc("sf_grad_scale", table, chunks, tail=[ctypes.c_void_p(FAKE + 4)]) == A
    assert _rc("sf_grad_clamp", table, chunks, tail=[None]) == E


def _param(n=8, grad=True, dtype=torch.float32):
    p = torch.nn.Parameter(torch.zeros(n, dtype=dtype))
    if grad:
        p.grad = torch.ones(n, dtype=dtype)
    return p


def test_hipgradclip_refuses_bad_arguments():
    from slowfast.models.step_tail import HipGradClip
    p = _param()
    for nt in (1, 1.0, 3, 0, -2, "fro", None):
        with pytest.raises(ValueError, match="norm_type"):
            HipGradClip([p], max_norm=1.0, norm_type=nt)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(ValueError, match="max_norm"):
            HipGradClip([p], max_norm=bad)
        with pytest.raises(ValueError, match="clip_value"):
            HipGradClip([p], clip_value=bad)
    with pytest.raises(ValueError):
        HipGradClip([p])                                                   # neither: nothing to do
    for nt in (2, 2.0, float("inf"), math.inf, "inf"):
        HipGradClip([p], max_norm=1.0, norm_type=nt)
    c = HipGradClip([{"params": [p]}, {"params": [_param()]}], max_norm=1.0, clip_value=0.5)
    assert len(c._params) == 2 and c.max_norm == 1.0 and c.clip_value == 0.5 and c.norm_type == 2.0
    with pytest.raises(RuntimeError, match="clip_value alone"):
        HipGradClip([p], clip_value=1.0).guard


def test_hipgradclip_refuses_gradients_the_kernels_cannot_read():
    import sfhip
    from slowfast.models.step_tail import HipGradClip
    with pytest.raises(ValueError, match="float32"):
        HipGradClip([_param(dtype=torch.float64)], max_norm=1.0).clip()
    p = _param()
    p.grad = torch.ones(8, 2)[:, 0]
    assert not p.grad.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        HipGradClip([p], max_norm=1.0).clip()
    p = _param()
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3]]), torch.tensor([1.0, 2.0]), (8,))
    with pytest.raises(ValueError, match="sparse"):
        HipGradClip([p], max_norm=1.0).clip()
    # CPU gradients: there is no CPU fallback
    for kw in ({"max_norm": 1.0}, {"clip_value": 1.0}, {"max_norm": 1.0, "norm_type": float("inf")}):
        with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
            HipGradClip([_param()], **kw).clip()


def test_low_level_entries_refuse_cpu_tables():
    import sfhip
    from slowfast.models.step_tail import grad_clamp, grad_norm, grad_scale
    table, chunks = _tables()
    state, partials = torch.zeros(8), torch.zeros(chunks.shape[0], dtype=torch.float64)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        grad_norm(table, table.clone(), chunks, chunks.clone(), 2, partials, state)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        grad_scale(table, table.clone(), chunks, chunks.clone(), state)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        grad_clamp(table, table.clone(), chunks, chunks.clone(), torch.ones(1))


def test_empty_parameter_lists_are_a_no_op():
    import sfhip
    from slowfast.models.step_tail import HipGradClip
    calls = sfhip.CALLS
    assert HipGradClip([], max_norm=1.0).clip() is None
    assert HipGradClip([_param(grad=False), _param(grad=False)], max_norm=1.0, clip_value=2.0).clip() is None
    assert sfhip.CALLS == calls


def test_construct_hip_grad_clip_reads_the_upstream_keys():
    from slowfast.config.defaults import get_cfg
    from slowfast.models.step_tail import HipGradClip, construct_hip_grad_clip
    model = torch.nn.Linear(3, 2)
    cfg = get_cfg()
    assert construct_hip_grad_clip(model, cfg) is None
    solver = dict(cfg.SOLVER)
    cfg = type("C", (), {"SOLVER": dict(solver, CLIP_GRAD_L2NORM=None, CLIP_GRAD_VAL=None)})()
    assert construct_hip_grad_clip(model, cfg) is None
    cfg.SOLVER = dict(solver, CLIP_GRAD_L2NORM=1.5)
    c = construct_hip_grad_clip(model, cfg, ring="r")
    assert isinstance(c, HipGradClip) and (c.max_norm, c.clip_value, c.norm_type, c.ring) == (1.5, None, 2.0, "r")
    assert [id(p) for p in c._params] == [id(p) for p in model.parameters()]
    cfg.SOLVER = dict(solver, CLIP_GRAD_L2NORM=2.0, CLIP_GRAD_VAL=0.25)
    c = construct_hip_grad_clip(model, cfg)
    assert (c.max_norm, c.clip_value) == (2.0, 0.25)
    cfg.SOLVER = dict(solver, CLIP_GRAD_VAL=-1.0)
    with pytest.raises(ValueError, match="clip_value"):
        construct_hip_grad_clip(model, cfg)


# ------------------------------------------------------------------------------------------------ meter drain
class _Cfg(object):
    LOG_PERIOD, NUM_GPUS = 3, 1
    SOLVER = type("S", (), {"MAX_EPOCH": 2})()
    DATA = type("D", (), {"MULTI_LABEL": False})()


def _write_step(ring, loss, norm):
    row = int(ring.counter[0]) % ring.cap
    ring.rows[row] = torch.tensor([loss, 50.0, 25.0, 0.0, 4.0, 0.0, 0.0, norm])
    ring.counter += 1


def _logged(meter, norms):
    meter.iter_tic()
    for i, g in enumerate(norms):
        _write_step(meter.ring, 1.0 + i, g)
        meter.iter_toc()
        meter.update_stats(0.1)
        s = meter.log_iter_stats(0, i)
    return s


def test_meter_folds_the_grad_norm_column_only_when_asked():
    from slowfast.utils.meters import DeviceTrainMeter
    norms = [3.5, 0.25, 7.0]
    plain = _logged(DeviceTrainMeter(10, _Cfg(), device="cpu"), norms)
    with_norm = _logged(DeviceTrainMeter(10, _Cfg(), device="cpu", grad_norm=True), norms)
    assert "grad_norm" not in plain
    assert with_norm["grad_norm"] == np.median(norms) == 3.5
    drop = ("time_diff", "eta", "gpu_mem", "grad_norm")
    assert {k: v for k, v in with_norm.items() if k not in drop} == {k: v for k, v in plain.items() if k not in drop}
    # a norm that is not finite under a clear loss flag: the same warning — but only for the meter that was asked
    for bad in (float("nan"), float("inf")):
        m = DeviceTrainMeter(10, _Cfg(), device="cpu", grad_norm=True)
        _write_step(m.ring, 1.0, bad)
        with pytest.raises(RuntimeWarning, match="Got NaN losses"):
            m.drain()
        m = DeviceTrainMeter(10, _Cfg(), device="cpu")
        _write_step(m.ring, 1.0, bad)
        assert m.drain() == 1
