"""Host side of the averaged weights (sf_avg_update, sf_avg_exchange, slowfast/models/weight_avg.py): the exports, the
audit's hot list, every refusal of the two entry points (checked before any launch, so callable without a GPU), the
table builder's tiling, HipAveragedModel's checkpoints against torch.optim.swa_utils.AveragedModel on a CPU module, and
construct_hip_ema on the default config."""
import contextlib
import ctypes
import io
import os

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from _util import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7f0000001000  # a non-null, 16-byte aligned "device address": a refused call never dereferences it


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _numels():
    C = _chunk()
    return [C, 1, 3, 4, 5, C - 1, C + 1, 2 * C + 1]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _entries():
    out, addr = [], FAKE
    for i, n in enumerate(_numels()):
        out.append((addr, addr + 0x10000000, n, i % 2))  # kinds 0 and 1 in turn
        addr += 4 * n
    out.append((FAKE + 0x20000000, FAKE + 0x30000000, 1, 2))  # one int64 word
    return out


def _good():
    from slowfast.models.weight_avg import build_avg_tables
    return build_avg_tables(_entries(), _chunk())


def _update_rc(table, chunks, mode=0, w=0.001, null=None, counts=None, count=FAKE, hyper=FAKE, no_hyper_host=False):
    import sfhip
    dev = ctypes.c_void_p(FAKE)
    hyper_host = torch.tensor([w], dtype=torch.float32)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], mode,
            None if no_hyper_host else _vp(hyper_host), ctypes.c_void_p(hyper) if hyper else None,
            ctypes.c_void_p(count) if count else None, None, None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return sfhip.lib().sf_avg_update(*args)


def _exchange_rc(table, chunks, op=0, null=None, counts=None):
    import sfhip
    dev = ctypes.c_void_p(FAKE)
    args = [_vp(table), dev, table.shape[0], _vp(chunks), dev, chunks.shape[0], op, None]
    if null is not None:
        args[null] = None
    for k, v in (counts or {}).items():
        args[k] = v
    return sfhip.lib().sf_avg_exchange(*args)


def _tampered_chunks(chunks):
    C = _chunk()
    return [m(chunks.clone()).contiguous() for m in (
        lambda c: c[:-1], lambda c: torch.cat([c, c[-1:]]), lambda c: c.flip(0), lambda c: torch.cat([c[:1], c]),
        lambda c: torch.where(c == C, torch.tensor(C - 4), c),           # a start off the chunk grid
        lambda c: torch.cat([c[:5], torch.tensor([[4, C]]), c[5:]]))]    # a chunk past its tensor's end


def test_symbols_are_exported_and_the_kernels_are_on_the_hot_list():
    import sfhip
    assert "sf_avg_update" in sfhip.EXPORTS and "sf_avg_exchange" in sfhip.EXPORTS
    lib = sfhip.lib()
    assert lib.sf_avg_update is not None and lib.sf_avg_exchange is not None
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    assert "avg_update_kernel" in audit.HOT and "avg_exchange_kernel" in audit.HOT
    assert not any(e.startswith("avg_") for e in audit.EXEMPT)


def test_table_builder_tiles_the_tensors():
    table, chunks = _good()
    C, numels = _chunk(), _numels() + [1]
    assert table.dtype == torch.int64 and tuple(table.shape) == (9, 4)
    assert table[:, 2].tolist() == numels and table[:, 3].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 2]
    want = []
    for i, n in enumerate(numels):
        want += [[i, s] for s in range(0, n, C)]
    assert chunks.tolist() == want and len(want) == 12


def test_avg_update_refusals():
    import sfhip
    table, chunks = _good()
    E, A = sfhip.SF_EINVAL, sfhip.SF_EALIGN
    for null in (0, 1, 3, 4, 7, 8, 9):  # every pointer but the guard (7, 8: hyper_host and hyper, needed in mode 0)
        assert _update_rc(table, chunks, null=null) == E, null
    for pos in (2, 5):  # n_tensors, n_chunks
        for v in (0, -1):
            assert _update_rc(table, chunks, counts={pos: v}) == E, (pos, v)
    for mode in (-1, 3, 7):
        assert _update_rc(table, chunks, mode=mode) == E, mode
    for w in (-0.001, 1.001, float("nan"), float("inf"), -float("inf")):  # 1 - decay outside [0, 1] or not finite
        assert _update_rc(table, chunks, mode=0, w=w) == E, w

    def bad_row(col, value, row=4):
        t = table.clone()
        t[row, col] = value
        return _update_rc(t, chunks)
    for col in (0, 1):  # average, source: null; not even a float's alignment
        assert bad_row(col, 0) == E, col
        assert bad_row(col, FAKE + 2) == A and bad_row(col, FAKE + 1) == A, col
        assert bad_row(col, FAKE + 4, row=8) == A, col  # a word wants 8 bytes
    assert bad_row(2, 0) == E and bad_row(2, -5) == E                        # numel <= 0
    assert bad_row(3, 3) == E and bad_row(3, -1) == E                        # kind outside 0..2
    for c in _tampered_chunks(chunks):
        assert _update_rc(table, c) == E
    t = table.clone()
    t[6, 2] = _chunk()  # a numel that no longer agrees with the chunks
    assert _update_rc(t, chunks) == E
    assert _update_rc(table, chunks, count=FAKE + 4) == A


def test_avg_exchange_refusals():
    import sfhip
    table, chunks = _good()
    E, A = sfhip.SF_EINVAL, sfhip.SF_EALIGN
    for null in (0, 1, 3, 4):
        assert _exchange_rc(table, chunks, null=null) == E, null
    for pos in (2, 5):
        for v in (0, -1):
            assert _exchange_rc(table, chunks, counts={pos: v}) == E, (pos, v)
    for op in (-1, 3):
        assert _exchange_rc(table, chunks, op=op) == E, op

    def bad_row(col, value, row=4):
        t = table.clone()
        t[row, col] = value
        return _exchange_rc(t, chunks)
    for col in (0, 1):
        assert bad_row(col, 0) == E and bad_row(col, FAKE + 2) == A and bad_row(col, FAKE + 4, row=8) == A, col
    assert bad_row(2, 0) == E and bad_row(3, 3) == E and bad_row(3, -1) == E
    for c in _tampered_chunks(chunks):
        assert _exchange_rc(table, c) == E


def test_cpu_tables_raise_sfhip_error():
    import sfhip
    from slowfast.models import weight_avg as wa
    table, chunks = _good()
    count = torch.zeros((), dtype=torch.int64)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        wa.avg_update(table, table.clone(), chunks, chunks.clone(), wa.MODE_MEAN, count)
    with pytest.raises(sfhip.SfhipError, match="no CPU fallback"):
        wa.avg_exchange(table, table.clone(), chunks, chunks.clone(), wa.OP_SWAP)
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    ema = wa.HipAveragedModel(net, decay=0.9)
    with pytest.raises(sfhip.SfhipError, match="GPU only"):  # a CPU model: refused, not averaged by torch
        ema.update_parameters()
    with pytest.raises(sfhip.SfhipError, match="GPU only"):
        ema.swap()


def _net(seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.ReLU(),
                              torch.nn.Conv2d(4, 5, 1, bias=False), torch.nn.BatchNorm2d(5))
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_()
                m.running_var.uniform_(0.5, 2.0)
                m.num_batches_tracked.fill_(seed)
    return net


@pytest.mark.parametrize("decay", [None, 0.9])
def test_state_dict_round_trips_with_torchs_averaged_model(decay):
    from slowfast.models.weight_avg import HipAveragedModel
    net = _net(3)
    names = [n for n, _ in list(net.named_parameters()) + list(net.named_buffers())]
    mine = HipAveragedModel(net, decay=decay)
    assert list(mine.averaged) == names  # chain(named_parameters(), named_buffers())
    assert all(tuple(v.shape) == tuple(t.shape) and v.dtype == t.dtype and torch.equal(v, t) for v, t in zip(
        mine.averaged.values(), list(net.parameters()) + list(net.buffers())))  # starts as a copy, as the deep copy does
    floats = [v for v in mine.averaged.values() if v.dtype == torch.float32]
    assert all(v.data_ptr() % 16 == 0 for v in floats)
    assert len({v.untyped_storage().data_ptr() for v in floats}) == 1  # one allocation
    assert mine.n_averaged.dtype == torch.int64 and mine.n_averaged.dim() == 0
    kw = {} if decay is None else {"multi_avg_fn": get_ema_multi_avg_fn(decay)}
    theirs = AveragedModel(_net(4), use_buffers=True, **kw)
    theirs.update_parameters(_net(5))
    theirs.update_parameters(_net(6))
    a, b = mine.state_dict(), theirs.state_dict()
    assert list(a) == list(b) and list(a)[0] == "n_averaged" and all(k.startswith("module.") for k in list(a)[1:])
    assert all(tuple(a[k].shape) == tuple(b[k].shape) and a[k].dtype == b[k].dtype for k in a)
    # theirs -> mine
    mine.load_state_dict(b)
    assert int(mine.n_averaged) == 2
    assert all(torch.equal(mine.state_dict()[k], b[k]) for k in b)
    assert all(torch.equal(mine.averaged[k[len("module."):]], v) for k, v in b.items() if k != "n_averaged")
    # mine -> theirs
    other = HipAveragedModel(_net(7), decay=decay)
    other.n_averaged.fill_(11)
    want = {k: v.clone() for k, v in other.state_dict().items()}
    theirs.load_state_dict(other.state_dict(), strict=True)
    assert int(theirs.n_averaged) == 11 and all(torch.equal(theirs.state_dict()[k], want[k]) for k in want)
    # a missing key, an unexpected key and a wrong shape raise, naming the key
    sd = dict(b)
    sd.pop("module.3.weight")
    with pytest.raises(KeyError, match="module.3.weight"):
        mine.load_state_dict(sd)
    with pytest.raises(KeyError, match="module.9.weight"):
        mine.load_state_dict(dict(b, **{"module.9.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="module.1.running_var"):
        mine.load_state_dict(dict(b, **{"module.1.running_var": torch.zeros(5)}))


def test_hip_averaged_model_refuses_what_the_kernel_does_not_do():
    from slowfast.models.weight_avg import HipAveragedModel
    with pytest.raises(ValueError, match="float32 only"):
        HipAveragedModel(torch.nn.Linear(3, 2).double())
    bad = torch.nn.Linear(3, 2)
    bad.weight = torch.nn.Parameter(torch.zeros(3, 2).t())
    with pytest.raises(ValueError, match="must be contiguous"):
        HipAveragedModel(bad)
    for d in (-0.1, 1.1, float("nan"), "x"):
        with pytest.raises(ValueError):
            HipAveragedModel(torch.nn.Linear(3, 2), decay=d)
    ema = HipAveragedModel(torch.nn.Linear(3, 2), decay=0.5)
    assert ema.mode == 0 and ema.set_decay(0.5) is False
    with pytest.raises(ValueError):
        ema.set_decay(2.0)
    swa = HipAveragedModel(torch.nn.Linear(3, 2))
    assert swa.mode == 1
    with pytest.raises(ValueError, match="decay=None"):
        swa.set_decay(0.9)
    kinds = HipAveragedModel(_net(1), decay=0.9, use_buffers=False)._kinds
    assert kinds == [0] * 7 + [1, 1, 2, 1, 1, 2]  # parameters averaged, float buffers copied, counts copied
    assert HipAveragedModel(_net(1), decay=0.9)._kinds == [0] * 7 + [0, 0, 2, 0, 0, 2]


def test_construct_hip_ema_reads_the_config_with_get():
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    from slowfast.models.weight_avg import HipAveragedModel, construct_hip_ema
    z, meta = load_case("slow_r18_s64")
    cfg = get_cfg()
    cfg.merge_from_other_cfg(meta["cfg_dump"])
    cfg.NUM_GPUS = 0
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    assert "EMA_ON" not in cfg.SOLVER  # config/defaults.py keeps the reference's key set
    assert construct_hip_ema(model, cfg) is None
    cfg.SOLVER.EMA_ON = False
    assert construct_hip_ema(model, cfg) is None
    cfg.SOLVER.EMA_ON = True
    ema = construct_hip_ema(model, cfg)
    assert type(ema) is HipAveragedModel and ema.decay == 0.999 and ema.use_buffers is True and ema.model is model
    assert list(ema.averaged) == [n for n, _ in list(model.named_parameters()) + list(model.named_buffers())]
    cfg.SOLVER.EMA_DECAY, cfg.SOLVER.EMA_USE_BUFFERS = 0.9, False
    ema = construct_hip_ema(model, cfg)
    assert ema.decay == 0.9 and ema.use_buffers is False
