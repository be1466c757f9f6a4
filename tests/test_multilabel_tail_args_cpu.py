"""Host side of the multi-label / detection training tail (sf_bce, sf_adam_step, HipBCE, HipAdam, DeviceTrainMeter
under DATA.MULTI_LABEL): every refusal of the two entry points (checked before any launch, so callable without a GPU),
the Adam address table and its chunk tiling, construct_hip_solver's "adam" branch, get_hip_loss_func, and the
meter's multi-label drain against the reference's own TrainMeter
(tests/golden/make_golden_train_meter_multilabel.py -> train_meter_multilabel_stats.json) — alone and as two gloo
ranks."""
import contextlib
import ctypes
import io
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from _util import GOLDEN, load_case

FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _numels():
    C = _chunk()
    return [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1]


# ------------------------------------------------------------------------------------------------ sf_bce
def _bce_rc(N=4, K=10, ldx=None, ldy=None, from_logits=0, cap=3, null=None):
    import sfhip
    L = sfhip.lib()
    p = ctypes.c_void_p(FAKE)
    cnt = ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    args = [p, K if ldx is None else ldx, p, K if ldy is None else ldy, N, K, from_logits, p, p, cnt, cap, p, None]
    if null is not None:
        args[null] = None
    return L.sf_bce(*args)


def test_bce_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    for null in (0, 2, 7, 8, 9, 11):  # x, y, dx, ring, counter, loss_out
        assert _bce_rc(null=null) == E, null
    assert _bce_rc(N=0) == E and _bce_rc(N=-1) == E
    assert _bce_rc(K=0) == E and _bce_rc(K=-3) == E
    assert _bce_rc(ldx=9) == E and _bce_rc(ldy=9) == E
    assert _bce_rc(cap=0) == E and _bce_rc(cap=-1) == E
    assert _bce_rc(from_logits=2) == E and _bce_rc(from_logits=-1) == E


def test_bce_python_entry_refuses_cpu_tensors_and_empty_batches():
    import sfhip
    from slowfast.models import step_tail as st
    ring = st.StatsRing(2, device="cpu")
    out = torch.zeros(2)
    with pytest.raises(sfhip.SfhipError):
        st.bce(torch.rand(3, 5), torch.rand(3, 5), False, ring, out)
    for cls in (st.HipBCE, st.HipBCEWithLogits):
        with pytest.raises(ValueError, match="empty batch"):
            cls(ring)(torch.zeros(0, 80), torch.zeros(0, 80))


# ------------------------------------------------------------------------------------------------ sf_adam_step
def _entries(numels, groups=2):
    out, addr = [], FAKE
    for i, n in enumerate(numels):
        out.append((addr, addr + 0x10000000, addr + 0x20000000, addr + 0x30000000, FAKE + 0x40000000 + 16 * i, n,
                    i % groups))
        addr += 4 * n
    return out


def test_adam_table_builder_rows_and_chunk_tiling():
    from slowfast.models.step_tail import build_adam_tables
    C = _chunk()
    assert C > 0 and C % 4 == 0
    numels = _numels()
    entries = _entries(numels)
    table, chunks = build_adam_tables(entries, C)
    assert table.dtype == torch.int64 and chunks.dtype == torch.int64 and tuple(table.shape) == (len(numels), 7)
    assert table.tolist() == [list(e) for e in entries]
    want = []
    for i, n in enumerate(numels):
        want += [[i, s] for s in range(0, n, C)]
    assert chunks.tolist() == want
    assert [sum(1 for c in want if c[0] == i) for i in range(len(numels))] == [1, 1, 1, 1, 1, 1, 2, 3]
    for i, s in want:
        assert 0 <= s < numels[i] and s % C == 0


def _adam_rc(table, chunks, hyper, n_groups=None, guard=None, zero_grad=0, null=None, counts=None):
    import sfhip
    L = sfhip.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    dev = ctypes.c_void_p(FAKE)
    args = [vp(table), dev, table.shape[0], vp(chunks), dev, chunks.shape[0], vp(hyper), dev,
            hyper.shape[0] if n_groups is None else n_groups, guard, zero_grad, None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return L.sf_adam_step(*args)


def _good_tables():
    from slowfast.models.step_tail import build_adam_tables
    table, chunks = build_adam_tables(_entries(_numels()), _chunk())
    hyper = torch.tensor([[0.1, 0.9, 0.999, 1e-8, 1e-4], [0.1, 0.9, 0.999, 1e-8, 0.0]], dtype=torch.float64)
    return table, chunks, hyper


def test_adam_step_refusals():
    import sfhip
    table, chunks, hyper = _good_tables()
    E = sfhip.SF_EINVAL
    for null in (0, 1, 3, 4, 6, 7):  # every pointer but the guard
        assert _adam_rc(table, chunks, hyper, null=null) == E, null
    for pos in (2, 5, 8):  # n_tensors, n_chunks, n_groups
        for v in (0, -1):
            assert _adam_rc(table, chunks, hyper, counts={pos: v}) == E, (pos, v)
    assert _adam_rc(table, chunks, hyper, zero_grad=2) == E and _adam_rc(table, chunks, hyper, zero_grad=-1) == E

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _adam_rc(t, chunks, hyper)
    for col in range(5):  # parameter, gradient, exp_avg, exp_avg_sq, step: null, or not even a float's alignment
        assert bad_row(col, 0) == E, col
        assert bad_row(col, FAKE + 2) == E and bad_row(col, FAKE + 1) == E, col
    assert bad_row(5, 0) == E and bad_row(5, -5) == E                       # numel <= 0
    assert bad_row(6, 2) == E and bad_row(6, -1) == E                       # group out of range

    def bad_hyper(col, value):
        h = hyper.clone()
        h[1, col] = value
        return _adam_rc(table, chunks, h)
    for col in range(5):
        assert bad_hyper(col, float("nan")) == E and bad_hyper(col, float("inf")) == E, col
    for col in (1, 2):  # a beta outside [0, 1): 1 - beta^t would not be positive
        assert bad_hyper(col, 1.0) == E and bad_hyper(col, -0.1) == E, col
    # tampered host chunks: anything that does not tile the tensors exactly
    C = _chunk()
    for mutate in (lambda c: c[:-1], lambda c: torch.cat([c, c[-1:]]), lambda c: c.flip(0),
                   lambda c: torch.cat([c[:1], c]),
                   lambda c: torch.where(c == C, torch.tensor(C - 4), c),           # a start off the chunk grid
                   lambda c: torch.cat([c[:5], torch.tensor([[4, C]]), c[5:]])):    # a chunk past its tensor's end
        c = mutate(chunks.clone()).contiguous()
        assert _adam_rc(table, c, hyper) == E
    # a tampered host table: a numel that no longer agrees with the chunks
    t = table.clone()
    t[6, 5] = C
    assert _adam_rc(t, chunks, hyper) == E


# ------------------------------------------------------------------------------------------------ Python side
def _model(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg), cfg


def test_construct_hip_solver_adam_split_and_state_dict_keys():
    from slowfast.models.step_tail import HipAdam, HipSGD, construct_hip_adam, construct_hip_optimizer, construct_hip_solver
    model, cfg = _model("slow_r18_s64")
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY, cfg.SOLVER.BASE_LR = 1e-4, 0.0, 0.003
    opt = construct_hip_solver(model, cfg)
    assert isinstance(opt, HipAdam) and isinstance(opt, torch.optim.Adam)
    assert isinstance(construct_hip_adam(model, cfg), HipAdam)
    # the reference's split (models/optimizer.py:26-51): "bn" in the name
    bn = [p for n, p in model.named_parameters() if "bn" in n]
    rest = [p for n, p in model.named_parameters() if "bn" not in n]
    assert len(bn) > 0 and len(rest) > 0 and len(opt.param_groups) == 2
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in bn]
    assert [id(p) for p in opt.param_groups[1]["params"]] == [id(p) for p in rest]
    assert opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[1]["weight_decay"] == 1e-4
    for g in opt.param_groups:
        assert g["lr"] == 0.003 and tuple(g["betas"]) == (0.9, 0.999) and g["eps"] == 1e-8 and not g["amsgrad"]
    ref = torch.optim.Adam([{"params": bn, "weight_decay": 0.0}, {"params": rest, "weight_decay": 1e-4}], lr=0.003,
                           betas=(0.9, 0.999), weight_decay=1e-4)
    a, b = opt.state_dict(), ref.state_dict()
    assert set(a) == set(b) and set(a["state"]) == set(b["state"]) == set()
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
    # state: one allocation, every view on 16 bytes
    assert len(opt._blocks) == 1
    for p in bn + rest:
        s = opt._slots[p]
        assert set(s) == {"exp_avg", "exp_avg_sq", "step"} and all(v.data_ptr() % 16 == 0 for v in s.values())
        assert s["exp_avg"].shape == p.shape == s["exp_avg_sq"].shape and s["step"].dim() == 0
    # the update kernel runs on the GPU only: a CPU model is refused at the step, not silently updated by torch
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError):
        opt.step()
    cfg.SOLVER.OPTIMIZING_METHOD = "sgd"
    assert isinstance(construct_hip_solver(model, cfg), HipSGD)
    cfg.SOLVER.OPTIMIZING_METHOD = "rmsprop"
    for construct in (construct_hip_solver, construct_hip_optimizer):
        with pytest.raises(NotImplementedError, match="Does not support rmsprop optimizer"):
            construct(model, cfg)


def test_hipadam_refuses_what_the_kernel_does_not_do():
    from slowfast.models.step_tail import HipAdam
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"amsgrad": True}, {"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError):
            HipAdam([p], lr=0.1, **kw)
    with pytest.raises(ValueError):
        HipAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError):  # torch's own check survives
        HipAdam([p], lr=0.1, betas=(1.0, 0.999))
    opt = HipAdam([p], lr=0.1)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))], "amsgrad": True})
    sd = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=0.1, amsgrad=True).state_dict()
    with pytest.raises(ValueError):
        HipAdam([p], lr=0.1).load_state_dict(sd)
    sd = torch.optim.Adam([torch.nn.Parameter(torch.zeros(4))], lr=0.1, maximize=True).state_dict()
    with pytest.raises(ValueError):
        HipAdam([p], lr=0.1).load_state_dict(sd)


def test_get_hip_loss_func_maps_the_reference_names():
    from slowfast.models import step_tail as st
    ring = st.StatsRing(2, device="cpu")

    def cfg(name):
        return type("C", (), {"MODEL": type("M", (), {"LOSS_FUNC": name})(), "TRAIN": type("T", (), {"TOPK": 5})()})()
    ce = st.get_hip_loss_func(cfg("cross_entropy"), ring)
    assert type(ce) is st.HipCrossEntropy and ce.topk == 5 and ce.ring is ring
    a, b = st.get_hip_loss_func(cfg("bce"), ring), st.get_hip_loss_func(cfg("bce_logit"), ring)
    assert type(a) is st.HipBCE and not a.from_logits and a.ring is ring
    assert type(b) is st.HipBCEWithLogits and b.from_logits and b.ring is ring
    with pytest.raises(NotImplementedError, match="Loss focal is not supported"):
        st.get_hip_loss_func(cfg("focal"), ring)


# ------------------------------------------------------------------------------------------------ meter drain
class _Cfg(object):
    def __init__(self, case):
        self.LOG_PERIOD, self.NUM_GPUS = case["log_period"], case["num_gpus"]
        self.SOLVER = type("S", (), {"MAX_EPOCH": case["max_epoch"]})()
        self.DATA = type("D", (), {"MULTI_LABEL": True})()


def _golden():
    with open(os.path.join(GOLDEN, "train_meter_multilabel_stats.json")) as f:
        return json.load(f)


def _write_step(ring, i, case, flag=0.0, bad=0.0):
    """What sf_bce leaves for step i, by hand on a CPU ring."""
    row = int(ring.counter[0]) % ring.cap
    ring.rows[row] = torch.tensor([case["loss"][i], 0.0, 0.0, flag, case["mb_per_gpu"], bad, 1.0, 0.0])
    ring.counter += 1


def _run_case(case, world_cfg=None):
    from slowfast.utils.meters import DeviceTrainMeter
    cfg = _Cfg(case)
    if world_cfg is not None:
        cfg.NUM_GPUS = world_cfg
    m = DeviceTrainMeter(case["epoch_iters"], cfg, device="cpu")
    assert m.ring.cap == case["log_period"]
    logged = []
    m.iter_tic()
    for i in range(len(case["loss"])):
        _write_step(m.ring, i, case)
        m.iter_toc()
        m.update_stats(case["lr"][i])
        s = m.log_iter_stats(case["cur_epoch"], i)
        if s is not None:
            logged.append(s)
        m.iter_tic()
    logged.append(m.log_epoch_stats(case["cur_epoch"]))
    return logged


def _same_stats(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        # the reference's keys and no others but the machine's fields: no top*_err, no epoch loss
        assert set(g) - {"time_diff", "eta", "gpu_mem", "RAM"} == set(w)
        assert {"time_diff", "eta", "gpu_mem"} <= set(g)
        assert "top1_err" not in g and "top5_err" not in g
        assert ("loss" in g) == (g["_type"] == "train_iter")
        for k, v in w.items():
            if isinstance(v, float):
                assert float(g[k]) == v, (k, g[k], v)  # the reference's arithmetic on the same values: equal floats
            else:
                assert g[k] == v, (k, g[k], v)


def test_multilabel_meter_drain_matches_reference_train_meter():
    case = _golden()["period4"]
    assert [s["_type"] for s in case["logged"]] == ["train_iter", "train_iter", "train_epoch"]
    _same_stats(_run_case(case), case["logged"])


def test_multilabel_meter_drain_errors():
    from slowfast.utils.meters import DeviceTrainMeter
    case = _golden()["period4"]
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    _write_step(m.ring, 0, case)
    _write_step(m.ring, 1, case, flag=1.0)
    with pytest.raises(RuntimeWarning, match="Got NaN losses"):
        m.drain()
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    _write_step(m.ring, 0, case, bad=2.0)
    with pytest.raises(ValueError, match=r"target or probability outside \[0, 1\]"):
        m.drain()
    # a cross-entropy row keeps its own wording
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    m.ring.rows[0] = torch.tensor([1.0, 50.0, 25.0, 0.0, 8.0, 1.0, 0.0, 0.0])
    m.ring.counter += 1
    with pytest.raises(ValueError, match=r"label\(s\) outside \[0, classes\)"):
        m.drain()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _drain_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "efficient-slowfast_amd"), here):
        sys.path.insert(0, p)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        case = _golden()["period3_world2"]
        # rank 0 holds zeros and rank 1 twice the recorded losses: only the all-reduced mean is the recorded sequence
        # (doubling and halving are exact in float32)
        mine = dict(case)
        mine["loss"] = [2.0 * rank * v for v in case["loss"]]
        got = _run_case(mine, world_cfg=world)
        if rank == 0:
            torch.save(got, out)
    finally:
        dist.destroy_process_group()


def test_multilabel_meter_drain_reduces_over_two_ranks(tmp_path):
    out = str(tmp_path / "stats.pt")
    mp.spawn(_drain_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    case = _golden()["period3_world2"]
    _same_stats(torch.load(out, weights_only=False), case["logged"])
