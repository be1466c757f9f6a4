"""Host side of the large-batch optimizers (sf_adamw_step, sf_lars_ratios, sf_lars_sgd_step, HipAdamW, HipLARS): every
refusal of the three entry points (checked before any launch, so callable without a GPU), the Python refusals,
construct_hip_solver's "adamw" and LARS_ON branches, and the float64 reference wrapper (tests/_lars_ref.py) against a
three-element case worked by hand."""
import contextlib
import ctypes
import io

import pytest
import torch

from _lars_ref import LarsRef
from _util import load_case

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _numels():
    C = _chunk()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _tampered_chunks(chunks):
    C = _chunk()
    return [m(chunks.clone()).contiguous() for m in (
        lambda c: c[:-1], lambda c: torch.cat([c, c[-1:]]), lambda c: c.flip(0), lambda c: torch.cat([c[:1], c]),
        lambda c: torch.where(c == C, torch.tensor(C - 4), c),           # a start off the chunk grid
        lambda c: torch.cat([c[:5], torch.tensor([[4, C]]), c[5:]]))]    # a chunk past its tensor's end


# ------------------------------------------------------------------------------------------------ sf_adamw_step
def _adam_entries(numels, groups=2):
    out, addr = [], FAKE
    for i, n in enumerate(numels):
        out.append((addr, addr + 0x10000000, addr + 0x20000000, addr + 0x30000000, FAKE + 0x40000000 + 16 * i, n,
                    i % groups))
        addr += 4 * n
    return out


def _adamw_rc(table, chunks, hyper, guard=None, zero_grad=0, null=None, counts=None, symbol="sf_adamw_step"):
    import sfhip
    dev = ctypes.c_void_p(FAKE)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], _vp(hyper), dev, hyper.shape[0], guard,
            zero_grad, None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return getattr(sfhip.lib(), symbol)(*args)


def test_adamw_step_refusals_are_adam_steps():
    import sfhip
    from slowfast.models.step_tail import build_adam_tables
    table, chunks = build_adam_tables(_adam_entries(_numels()), _chunk())
    hyper = torch.tensor([[0.1, 0.9, 0.999, 1e-8, 1e-4], [0.1, 0.9, 0.999, 1e-8, 0.0]], dtype=torch.float64)
    E = sfhip.SF_EINVAL
    for null in (0, 1, 3, 4, 6, 7):  # every pointer but the guard
        assert _adamw_rc(table, chunks, hyper, null=null) == E, null
    for pos in (2, 5, 8):  # n_tensors, n_chunks, n_groups
        for v in (0, -1):
            assert _adamw_rc(table, chunks, hyper, counts={pos: v}) == E, (pos, v)
    assert _adamw_rc(table, chunks, hyper, zero_grad=2) == E and _adamw_rc(table, chunks, hyper, zero_grad=-1) == E

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _adamw_rc(t, chunks, hyper)
    for col in range(5):  # parameter, gradient, exp_avg, exp_avg_sq, step: null, or not even a float's alignment
        assert bad_row(col, 0) == E, col
        assert bad_row(col, FAKE + 2) == E and bad_row(col, FAKE + 1) == E, col
    assert bad_row(5, 0) == E and bad_row(5, -5) == E                       # numel <= 0
    assert bad_row(6, 2) == E and bad_row(6, -1) == E                       # group out of range

    def bad_hyper(col, value):
        h = hyper.clone()
        h[1, col] = value
        return _adamw_rc(table, chunks, h)
    for col in range(5):
        assert bad_hyper(col, float("nan")) == E and bad_hyper(col, float("inf")) == E, col
    for col in (1, 2):  # a beta outside [0, 1)
        assert bad_hyper(col, 1.0) == E and bad_hyper(col, -0.1) == E, col
    for c in _tampered_chunks(chunks):
        assert _adamw_rc(table, c, hyper) == E
    t = table.clone()
    t[6, 5] = _chunk()  # a numel that no longer agrees with the chunks
    assert _adamw_rc(t, chunks, hyper) == E


# ------------------------------------------------------------------------------------------------ sf_lars_ratios
def _lars_entries(numels, groups=2):
    out, addr = [], FAKE
    for i, n in enumerate(numels):
        out.append((addr, addr + 0x10000000, n, i % groups, 1 if n == 3 else 0))
        addr += 4 * n
    return out


def _lars_good():
    from slowfast.models.step_tail import build_lars_tables
    table, chunks = build_lars_tables(_lars_entries(_numels()), _chunk())
    hyper = torch.tensor([[0.1, 1e-4, 1.0], [0.1, 0.0, 0.0], [0.02, 1e-8, 1.0]], dtype=torch.float32)
    return table, chunks, hyper


def _ratios_rc(table, chunks, hyper, null=None, counts=None, partials=FAKE, ratios=FAKE, state=FAKE):
    import sfhip
    dev = ctypes.c_void_p(FAKE)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], _vp(hyper), dev, hyper.shape[0] - 1,
            None, ctypes.c_void_p(partials), ctypes.c_void_p(ratios), ctypes.c_void_p(state), None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return sfhip.lib().sf_lars_ratios(*args)


def test_lars_table_builder_rows_first_chunks_and_tiling():
    table, chunks, _ = _lars_good()
    C, numels = _chunk(), _numels()
    assert table.dtype == torch.int64 and tuple(table.shape) == (len(numels), 6)
    assert table[:, 2].tolist() == numels and table[:, 3].tolist() == [i % 2 for i in range(len(numels))]
    assert table[:, 4].tolist() == [0, 1, 2, 3, 4, 5, 6, 8] and int(chunks.shape[0]) == 11
    assert table[:, 5].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    want = []
    for i, n in enumerate(numels):
        want += [[i, s] for s in range(0, n, C)]
    assert chunks.tolist() == want
    for t in range(len(numels)):  # a tensor's chunks are contiguous, from its first-chunk column on
        mine = [i for i, c in enumerate(want) if c[0] == t]
        assert mine == list(range(int(table[t, 4]), int(table[t, 4]) + len(mine)))


def test_lars_ratios_refusals():
    import sfhip
    table, chunks, hyper = _lars_good()
    E, A = sfhip.SF_EINVAL, sfhip.SF_EALIGN
    for null in (0, 1, 3, 4, 6, 7, 10, 11, 12):  # every pointer but guard_in
        assert _ratios_rc(table, chunks, hyper, null=null) == E, null
    for pos in (2, 5, 8):  # n_tensors, n_chunks, n_groups
        for v in (0, -1):
            assert _ratios_rc(table, chunks, hyper, counts={pos: v}) == E, (pos, v)

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _ratios_rc(t, chunks, hyper)
    for col in (0, 1):  # parameter, gradient: null, or not even a float's alignment
        assert bad_row(col, 0) == E and bad_row(col, FAKE + 2) == E and bad_row(col, FAKE + 1) == E, col
    assert bad_row(2, 0) == E and bad_row(2, -5) == E                        # numel <= 0
    assert bad_row(3, 2) == E and bad_row(3, -1) == E                        # group out of range
    assert bad_row(4, 2) == E and bad_row(4, 4) == E and bad_row(4, -1) == E  # not the running chunk count
    assert bad_row(5, 2) == E and bad_row(5, -1) == E                        # ignored flag outside {0, 1}

    def bad_hyper(row, value):
        h = hyper.clone()
        h[row, 2] = value
        return _ratios_rc(table, chunks, h)
    for row in (0, 1, 2):  # apply of either group, clip
        assert bad_hyper(row, 2.0) == E and bad_hyper(row, 0.5) == E and bad_hyper(row, -1.0) == E, row
        assert bad_hyper(row, float("nan")) == E, row
    for c in _tampered_chunks(chunks):
        assert _ratios_rc(table, c, hyper) == E
    t = table.clone()
    t[6, 2] = _chunk()  # a numel that no longer agrees with the chunks
    assert _ratios_rc(t, chunks, hyper) == E
    assert _ratios_rc(table, chunks, hyper, partials=FAKE + 4) == A and _ratios_rc(table, chunks, hyper, state=FAKE + 4) == A
    assert _ratios_rc(table, chunks, hyper, ratios=FAKE + 2) == E


# ------------------------------------------------------------------------------------------------ sf_lars_sgd_step
def _sgd_entries(numels, groups=2):
    out, addr = [], FAKE
    for i, n in enumerate(numels):
        out.append((addr, addr + 0x10000000, addr + 0x20000000, n, i % groups, 0))
        addr += 4 * n
    return out


def _lars_step_rc(table, chunks, hyper, zero_grad=0, null=None, counts=None):
    import sfhip
    dev = ctypes.c_void_p(FAKE)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], _vp(hyper), dev, hyper.shape[0], dev,
            None, zero_grad, None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return sfhip.lib().sf_lars_sgd_step(*args)


def test_lars_sgd_step_refusals():
    import sfhip
    from slowfast.models.step_tail import build_sgd_tables
    table, chunks = build_sgd_tables(_sgd_entries(_numels()), _chunk())
    hyper = torch.tensor([[0.1, 1e-4, 0.9, 0.0, 1.0], [0.1, 0.0, 0.9, 0.0, 0.0]], dtype=torch.float32)
    E = sfhip.SF_EINVAL
    for null in (0, 1, 3, 4, 6, 7, 9):  # every pointer but the guard; 9: ratios
        assert _lars_step_rc(table, chunks, hyper, null=null) == E, null
    for pos in (2, 5, 8):
        for v in (0, -1):
            assert _lars_step_rc(table, chunks, hyper, counts={pos: v}) == E, (pos, v)
    assert _lars_step_rc(table, chunks, hyper, zero_grad=2) == E and _lars_step_rc(table, chunks, hyper, zero_grad=-1) == E

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _lars_step_rc(t, chunks, hyper)
    for col in (0, 1):
        assert bad_row(col, 0) == E and bad_row(col, FAKE + 2) == E, col
    assert bad_row(2, FAKE + 2) == E and bad_row(2, 0) == E                  # momentum without a buffer
    assert bad_row(3, 0) == E and bad_row(3, -5) == E
    assert bad_row(4, 2) == E and bad_row(4, -1) == E
    assert bad_row(5, 2) == E and bad_row(5, -1) == E
    for c in _tampered_chunks(chunks):
        assert _lars_step_rc(table, c, hyper) == E


# ------------------------------------------------------------------------------------------------ Python side
def test_hipadamw_refuses_what_the_kernel_does_not_do():
    from slowfast.models.step_tail import HipAdam, HipAdamW
    p = torch.nn.Parameter(torch.zeros(4))
    assert HipAdamW._REFUSED == ("amsgrad", "maximize", "differentiable")
    assert "decoupled_weight_decay" in HipAdam._REFUSED  # HipAdam keeps refusing it
    with pytest.raises(ValueError):
        HipAdam([p], lr=0.1, decoupled_weight_decay=True)
    for kw in ({"amsgrad": True}, {"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError):
            HipAdamW([p], lr=0.1, **kw)
    with pytest.raises(ValueError):
        HipAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError):
        HipAdamW([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1)  # not contiguous
    with pytest.raises(ValueError):  # torch's own check survives
        HipAdamW([p], lr=0.1, betas=(1.0, 0.999))
    opt = HipAdamW([p], lr=0.1)
    assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 1e-2
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))], "amsgrad": True})
    sd = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(4))], lr=0.1, amsgrad=True).state_dict()
    with pytest.raises(ValueError):
        HipAdamW([p], lr=0.1).load_state_dict(sd)
    with pytest.raises(ValueError, match="use HipAdam"):  # coupled decay is HipAdam's kernel
        HipAdamW([p], lr=0.1).add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))],
                                               "decoupled_weight_decay": False})
    opt = HipAdamW([p], lr=0.1)
    p.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="GPU only"):  # a CPU parameter at step: refused, not updated by torch
        opt.step()


def test_hiplars_refuses_what_the_kernel_does_not_do():
    from slowfast.models.step_tail import HipLARS, HipSGD
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError):
            HipLARS([p], lr=0.1, **kw)
    for kw in ({"trust_coefficient": -1.0}, {"trust_coefficient": float("nan")}, {"eps": -1e-8}, {"eps": float("inf")}):
        with pytest.raises(ValueError):
            HipLARS([p], lr=0.1, **kw)
    with pytest.raises(ValueError):
        HipLARS([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError):
        HipLARS([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=0.1)  # not contiguous
    opt = HipLARS([{"params": [p]}, {"params": [torch.nn.Parameter(torch.zeros(3))], "apply_LARS": False}], lr=0.1,
                  momentum=0.9)
    assert isinstance(opt, HipSGD) and isinstance(opt, torch.optim.SGD)
    assert (opt.trust_coefficient, opt.clip, opt.eps, opt.ignore_1d_param) == (0.02, True, 1e-8, False)
    assert [g["apply_LARS"] for g in opt.param_groups] == [True, False]
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    assert opt.param_groups[2]["apply_LARS"] is True
    # the state dict is torch.optim.SGD's: it loads there, and an SGD one loads here without losing the switches
    ref = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(n))]} for n in (4, 3, 2)], lr=0.3, momentum=0.9)
    ref.load_state_dict(opt.state_dict())
    assert [g["lr"] for g in ref.param_groups] == [0.1, 0.1, 0.1]
    ref.param_groups[0]["lr"] = 0.7
    sd = ref.state_dict()
    for g in sd["param_groups"]:
        g.pop("apply_LARS")  # what torch.optim.SGD itself would have saved
    opt.load_state_dict(sd)
    assert [g["apply_LARS"] for g in opt.param_groups] == [True, False, True] and opt.param_groups[0]["lr"] == 0.7
    # the hyper row: sf_lars_sgd_step's [3][5], then sf_lars_ratios' [3 + 1][3]
    (row,) = opt._hyper_values()
    assert len(row) == 3 * 5 + 4 * 3 and row[15:18] == (0.7, 0.0, 1.0) and row[18:21] == (0.1, 0.0, 0.0)
    assert row[24:27] == (0.02, 1e-8, 1.0)
    with pytest.raises(RuntimeError, match="first step"):
        opt.guard
    p.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="GPU only"):  # a CPU parameter at step: refused, not updated by torch
        opt.step()


def _model(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg), cfg


def test_construct_hip_solver_adamw_and_lars():
    from slowfast.models.step_tail import (HipAdam, HipAdamW, HipLARS, HipSGD, construct_hip_optimizer,
                                           construct_hip_solver)
    model, cfg = _model("slow_r18_s64")
    assert "LARS_ON" not in cfg.SOLVER  # config/defaults.py keeps the reference's key set
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY, cfg.SOLVER.BASE_LR = 1e-4, 0.0, 0.003
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    bn = [p for n, p in model.named_parameters() if "bn" in n]
    rest = [p for n, p in model.named_parameters() if "bn" not in n]

    def split_ok(opt):
        assert len(opt.param_groups) == 2
        assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in bn]
        assert [id(p) for p in opt.param_groups[1]["params"]] == [id(p) for p in rest]
        assert opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[1]["weight_decay"] == 1e-4
        assert all(g["lr"] == 0.003 for g in opt.param_groups)

    cfg.SOLVER.OPTIMIZING_METHOD = "adamw"
    opt = construct_hip_solver(model, cfg)
    assert type(opt) is HipAdamW and isinstance(opt, torch.optim.AdamW) and not isinstance(opt, HipAdam)
    split_ok(opt)
    assert all(tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8 and not g["amsgrad"] for g in opt.param_groups)
    ref = torch.optim.AdamW([{"params": bn, "weight_decay": 0.0}, {"params": rest, "weight_decay": 1e-4}], lr=0.003)
    a, b = opt.state_dict(), ref.state_dict()
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]] and a["state"] == b["state"] == {}
    with pytest.raises(NotImplementedError, match="Does not support adamw optimizer"):
        construct_hip_optimizer(model, cfg)  # the sgd-only constructor keeps its messages

    cfg.SOLVER.OPTIMIZING_METHOD = "sgd"
    assert type(construct_hip_solver(model, cfg)) is HipSGD  # no LARS_ON key: as before
    cfg.SOLVER.LARS_ON = False
    assert type(construct_hip_solver(model, cfg)) is HipSGD
    cfg.SOLVER.LARS_ON = True
    opt = construct_hip_solver(model, cfg)
    assert type(opt) is HipLARS
    split_ok(opt)
    assert [g["apply_LARS"] for g in opt.param_groups] == [False, True]  # the BN group does not apply LARS
    assert all(g["momentum"] == 0.9 and g["nesterov"] and g["dampening"] == 0.0 for g in opt.param_groups)
    assert (opt.trust_coefficient, opt.clip) == (0.001, False)  # upstream's LARS(optimizer, 0.001, clip=False)
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    assert type(construct_hip_solver(model, cfg)) is HipAdam  # LARS is not applied to Adam
    with pytest.raises(NotImplementedError, match="construct_hip_optimizer builds sgd only"):
        construct_hip_optimizer(model, cfg)
    cfg.SOLVER.OPTIMIZING_METHOD = "rmsprop"
    for construct in (construct_hip_solver, construct_hip_optimizer):
        with pytest.raises(NotImplementedError, match="Does not support rmsprop optimizer"):
            construct(model, cfg)


# ------------------------------------------------------------------------------------------------ the reference wrapper
def _hand_case(clip, lr, p=(3.0, 0.0, 4.0), g=(0.0, 0.6, 0.8)):
    w = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    w.grad = torch.tensor(g, dtype=torch.float64)
    ref = LarsRef(torch.optim.SGD([w], lr=lr, weight_decay=0.1), trust_coefficient=0.02, clip=clip, eps=0.0)
    return w, ref


def test_reference_wrapper_against_a_case_worked_by_hand():
    # ||p|| = 5, ||g|| = 1, wd = 0.1: r = 0.02 * 5 / (1 + 5 * 0.1) = 1 / 15
    w, ref = _hand_case(False, 0.5)
    (r, wd_t), = ref.ratios()
    assert abs(r - 1.0 / 15.0) <= 1e-15 and wd_t == 0.1  # a handful of float64 roundings of numbers below 1
    ref.step()
    # g' = (g + 0.1 p) / 15 = (0.3, 0.6, 1.2) / 15 = (0.02, 0.04, 0.08);  p' = p - 0.5 g'
    assert torch.allclose(w.detach(), torch.tensor([2.99, -0.02, 3.96], dtype=torch.float64), rtol=0, atol=1e-15)
    assert ref.param_groups[0]["weight_decay"] == 0.1  # restored behind the step
    # clip: min(r / lr, 1) — lr 0.5: (1 / 15) / 0.5 = 2 / 15;  lr 0.05: 4 / 3 -> 1
    w, ref = _hand_case(True, 0.5)
    assert abs(ref.ratios()[0][0] - 2.0 / 15.0) <= 1e-15
    ref.step()
    assert torch.allclose(w.detach(), torch.tensor([2.98, -0.04, 3.92], dtype=torch.float64), rtol=0, atol=1e-15)
    w, ref = _hand_case(True, 0.05)
    assert ref.ratios() == [(1.0, 0.1)]
    ref.step()  # plain SGD with weight decay: p' = p - 0.05 (g + 0.1 p)
    assert torch.allclose(w.detach(), torch.tensor([2.985, -0.03, 3.94], dtype=torch.float64), rtol=0, atol=1e-15)
    # a zero gradient: r = 1 and NO decay — the tensor does not move
    w, ref = _hand_case(False, 0.5, g=(0.0, 0.0, 0.0))
    assert ref.ratios() == [(1.0, 0.0)]
    ref.step()
    assert torch.equal(w.detach(), torch.tensor([3.0, 0.0, 4.0], dtype=torch.float64))
    # a zero parameter: r = 1, no decay — p' = -lr g
    w, ref = _hand_case(False, 0.5, p=(0.0, 0.0, 0.0))
    assert ref.ratios() == [(1.0, 0.0)]
    ref.step()
    assert torch.equal(w.detach(), torch.tensor([-0.0, -0.3, -0.4], dtype=torch.float64))
    # apply_LARS False and ignore_1d_param: plain SGD with weight decay
    w, ref = _hand_case(False, 0.5)
    ref.param_groups[0]["apply_LARS"] = False
    assert ref.ratios() == [(1.0, 0.1)]
    w, ref = _hand_case(False, 0.5)
    ref.ignore_1d_param = True
    assert ref.ratios() == [(1.0, 0.1)]
    # a norm that is not finite: r = 1, wd_t = wd (the kernels raise the guard there)
    w, ref = _hand_case(False, 0.5, g=(0.0, float("nan"), 0.8))
    assert ref.ratios() == [(1.0, 0.1)]
