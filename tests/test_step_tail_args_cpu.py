"""Host side of the training-step tail (csrc/step_tail.hip, slowfast/models/step_tail.py, DeviceTrainMeter): the SGD
address table and its chunk tiling, every refusal of sf_ce_topk / sf_sgd_step (checked before any launch, so callable
without a GPU), construct_hip_optimizer's parameter split, HipSGD's state_dict, and the meter's drain against the
reference's own TrainMeter (tests/golden/make_golden_train_meter.py -> train_meter_stats.json) — alone and as two gloo
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


def _entries(numels, groups=2, momentum=True):
    out, addr = [], FAKE
    for i, n in enumerate(numels):
        out.append((addr, addr + 0x10000000, addr + 0x20000000 if momentum else 0, n, i % groups, 1 if i < 2 else 0))
        addr += 4 * n
    return out


def test_table_builder_rows_and_chunk_tiling():
    from slowfast.models.step_tail import build_sgd_tables
    C = _chunk()
    assert C > 0 and C % 4 == 0
    numels = _numels()
    entries = _entries(numels)
    table, chunks = build_sgd_tables(entries, C)
    assert table.dtype == torch.int64 and chunks.dtype == torch.int64
    assert table.tolist() == [list(e) for e in entries]
    want = []
    for i, n in enumerate(numels):
        want += [[i, s] for s in range(0, n, C)]
    assert chunks.tolist() == want
    # 1, 3, 4, 5, C - 1, C: one chunk each; C + 1: two; 2C + 1: three — no chunk straddles a tensor, none is empty
    assert [sum(1 for c in want if c[0] == i) for i in range(len(numels))] == [1, 1, 1, 1, 1, 1, 2, 3]
    for i, s in want:
        assert 0 <= s < numels[i] and s % C == 0


def _sgd_rc(table, chunks, hyper, n_groups=None, guard=None, zero_grad=0, null=None, counts=None):
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
    return L.sf_sgd_step(*args)


def _good_tables():
    from slowfast.models.step_tail import build_sgd_tables
    table, chunks = build_sgd_tables(_entries(_numels()), _chunk())
    hyper = torch.tensor([[0.1, 1e-4, 0.9, 0.0, 1.0], [0.1, 0.0, 0.9, 0.0, 1.0]], dtype=torch.float32)
    return table, chunks, hyper


def test_sgd_step_refusals():
    import sfhip
    table, chunks, hyper = _good_tables()
    E = sfhip.SF_EINVAL
    for null in (0, 1, 3, 4, 6, 7):  # every pointer but the guard
        assert _sgd_rc(table, chunks, hyper, null=null) == E, null
    for pos in (2, 5, 8):  # n_tensors, n_chunks, n_groups
        for v in (0, -1):
            assert _sgd_rc(table, chunks, hyper, counts={pos: v}) == E, (pos, v)
    assert _sgd_rc(table, chunks, hyper, zero_grad=2) == E and _sgd_rc(table, chunks, hyper, zero_grad=-1) == E

    def bad_row(col, value, row=3):
        t = table.clone()
        t[row, col] = value
        return _sgd_rc(t, chunks, hyper)
    assert bad_row(0, 0) == E and bad_row(1, 0) == E                      # null parameter / gradient address
    for col in (0, 1, 2):
        assert bad_row(col, FAKE + 2) == E and bad_row(col, FAKE + 1) == E  # not even a float's alignment
    assert bad_row(3, 0) == E and bad_row(3, -5) == E                       # numel <= 0
    assert bad_row(4, 2) == E and bad_row(4, -1) == E                       # group out of range
    assert bad_row(5, 2) == E                                               # first-step flag outside {0, 1}
    assert bad_row(2, 0) == E                                               # momentum group without a buffer
    # tables of groups without momentum (no buffer addresses), for the tiling refusals below; the accepted
    # momentum-0 launch itself is the GPU suite's 'plain' SGD mode
    h0 = hyper.clone()
    h0[:, 2] = 0.0
    h0[:, 4] = 0.0
    t = table.clone()
    t[:, 2] = 0
    # chunks that do not tile the tensors exactly
    C = _chunk()
    for mutate in (lambda c: c[:-1], lambda c: torch.cat([c, c[-1:]]), lambda c: c.flip(0),
                   lambda c: torch.cat([c[:1], c]),
                   lambda c: torch.where(c == C, torch.tensor(C - 4), c),           # a start off the chunk grid
                   lambda c: torch.cat([c[:5], torch.tensor([[4, C]]), c[5:]])):    # a chunk past its tensor's end
        c = mutate(chunks.clone()).contiguous()
        assert _sgd_rc(table, c, hyper) == E
        assert _sgd_rc(t, c, h0) == E


def _ce_rc(N=4, K=10, k_hi=5, ld=None, cap=3, null=None):
    import sfhip
    L = sfhip.lib()
    p = ctypes.c_void_p(FAKE)
    cnt = ctypes.cast(ctypes.c_void_p(FAKE), sfhip._pi)
    args = [p, K if ld is None else ld, p, N, K, k_hi, p, p, cnt, cap, p, None]
    if null is not None:
        args[null] = None
    return L.sf_ce_topk(*args)


def test_ce_topk_refusals():
    import sfhip
    E = sfhip.SF_EINVAL
    assert _ce_rc(k_hi=11) == E            # k_hi > K (torch.topk raises there)
    assert _ce_rc(k_hi=0) == E
    assert _ce_rc(N=0) == E and _ce_rc(N=-1) == E
    assert _ce_rc(K=0, k_hi=0) == E and _ce_rc(K=-3, k_hi=1) == E
    assert _ce_rc(cap=0) == E and _ce_rc(cap=-1) == E
    assert _ce_rc(ld=9) == E               # row stride below K
    for null in (0, 2, 6, 7, 8, 10):
        assert _ce_rc(null=null) == E, null


def _model(name):
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    z, meta = load_case(name)
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        return build_model(cfg), cfg


def test_parameter_split_and_state_dict_keys():
    from slowfast.models.step_tail import HipSGD, construct_hip_optimizer
    model, cfg = _model("dual_r50_s64")
    cfg.SOLVER.OPTIMIZING_METHOD = "sgd"
    cfg.SOLVER.MOMENTUM, cfg.SOLVER.NESTEROV, cfg.SOLVER.DAMPENING = 0.9, True, 0.0
    cfg.SOLVER.WEIGHT_DECAY, cfg.BN.WEIGHT_DECAY, cfg.SOLVER.BASE_LR = 1e-4, 0.0, 0.05
    opt = construct_hip_optimizer(model, cfg)
    assert isinstance(opt, HipSGD) and isinstance(opt, torch.optim.SGD)
    bn = [p for n, p in model.named_parameters() if "bn" in n]
    rest = [p for n, p in model.named_parameters() if "bn" not in n]
    assert len(bn) > 0 and len(rest) > 0 and len(opt.param_groups) == 2
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in bn]
    assert [id(p) for p in opt.param_groups[1]["params"]] == [id(p) for p in rest]
    assert opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[1]["weight_decay"] == 1e-4
    for g in opt.param_groups:
        assert (g["lr"], g["momentum"], g["nesterov"], g["dampening"]) == (0.05, 0.9, True, 0.0)
    # the same groups in torch's own optimizer: state_dict has the same keys, group by group
    ref = torch.optim.SGD([{"params": bn, "weight_decay": 0.0}, {"params": rest, "weight_decay": 1e-4}], lr=0.05,
                          momentum=0.9, weight_decay=1e-4, dampening=0.0, nesterov=True)
    a, b = opt.state_dict(), ref.state_dict()
    assert set(a) == set(b) and set(a["state"]) == set(b["state"])
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]
    assert [g["params"] for g in a["param_groups"]] == [g["params"] for g in b["param_groups"]]
    # momentum buffers: one allocation, every view on 16 bytes
    assert len(opt._blocks) == 1 and all(opt._slots[p].data_ptr() % 16 == 0 for p in bn + rest)
    # the update kernel runs on the GPU only: a CPU model is refused at the step, not silently updated by torch
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError):
        opt.step()
    cfg.SOLVER.OPTIMIZING_METHOD = "adam"
    with pytest.raises(NotImplementedError, match="torch"):
        construct_hip_optimizer(model, cfg)


def test_hipsgd_refuses_what_the_kernel_does_not_do():
    from slowfast.models.step_tail import HipSGD
    p = torch.nn.Parameter(torch.zeros(4))
    for kw in ({"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError):
            HipSGD([p], lr=0.1, **kw)
    with pytest.raises(ValueError):
        HipSGD([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError):  # torch's own check survives
        HipSGD([p], lr=0.1, nesterov=True)


# ------------------------------------------------------------------------------------------------ meter drain
class _Cfg(object):
    def __init__(self, case):
        self.LOG_PERIOD, self.NUM_GPUS = case["log_period"], case["num_gpus"]
        self.SOLVER = type("S", (), {"MAX_EPOCH": case["max_epoch"]})()
        self.DATA = type("D", (), {"MULTI_LABEL": False})()


def _golden():
    with open(os.path.join(GOLDEN, "train_meter_stats.json")) as f:
        return json.load(f)


def _write_step(ring, i, case, flag=0.0, bad=0.0):
    """What sf_ce_topk leaves for step i, by hand on a CPU ring."""
    row = int(ring.counter[0]) % ring.cap
    ring.rows[row] = torch.tensor([case["loss"][i], case["top1"][i], case["top5"][i], flag, case["mb_per_gpu"], bad,
                                   0.0, 0.0])
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
        assert set(w) <= set(g)
        assert {"time_diff", "eta", "gpu_mem"} <= set(g)
        for k, v in w.items():
            if isinstance(v, float):
                assert float(g[k]) == v, (k, g[k], v)  # the reference's arithmetic on the same values: equal floats
            else:
                assert g[k] == v, (k, g[k], v)


def test_meter_drain_matches_reference_train_meter():
    case = _golden()["period4"]
    _same_stats(_run_case(case), case["logged"])


def test_meter_drain_errors():
    from slowfast.utils.meters import DeviceTrainMeter, format_json_stats
    case = _golden()["period4"]
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    for i in range(5):  # one more step than the ring holds
        _write_step(m.ring, i, case)
    with pytest.raises(RuntimeError, match="ring"):
        m.drain()
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    _write_step(m.ring, 0, case)
    _write_step(m.ring, 1, case, flag=1.0)
    with pytest.raises(RuntimeWarning, match="Got NaN losses"):
        m.drain()
    m = DeviceTrainMeter(case["epoch_iters"], _Cfg(case), device="cpu")
    _write_step(m.ring, 0, case, bad=2.0)
    with pytest.raises(ValueError, match="label"):
        m.drain()
    # utils/logging.py:84-96: six decimals, sorted keys
    assert format_json_stats({"b": 0.5, "a": "1/2", "c": 3}) == 'json_stats: {"a": "1/2", "b": 0.500000, "c": 3}'


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
    from slowfast.utils.meters import DeviceTrainMeter
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        case = _golden()["period3_world2"]
        # rank 0 holds zeros and rank 1 twice the recorded values: only the all-reduced mean is the recorded sequence
        # (doubling and halving are exact in float32)
        mine = dict(case)
        for k in ("loss", "top1", "top5"):
            mine[k] = [2.0 * rank * v for v in case[k]]
        got = _run_case(mine, world_cfg=world)
        if rank == 0:
            torch.save(got, out)
    finally:
        dist.destroy_process_group()


def test_meter_drain_reduces_over_two_ranks(tmp_path):
    out = str(tmp_path / "stats.pt")
    mp.spawn(_drain_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    case = _golden()["period3_world2"]
    _same_stats(torch.load(out, weights_only=False), case["logged"])
