"""sf_avg_update and sf_avg_exchange on the GPU (csrc/weight_avg.hip) through slowfast/models/weight_avg.py, on the
eight-tensor problem of the optimizer tests: sizes C, 1, 3, 4, 5, C - 1, C + 1, 2 C + 1 (C = sf_sgd_chunk_elems())
packed tightly into one flat buffer — behind the one-element tensor some views are 4-byte- but not 16-byte-aligned —
plus one int64 word, sentinel margins around every buffer the kernels write.

Modes 0 and 1 are held against torch.optim.swa_utils.AveragedModel in float64 on the CPU; the bound is the project's
rule: what torch's own float32 foreach run on the GPU misses the same float64 values by, times 2.  Both errors are
printed per update; the figures measured on an MI355X are in profiles/weight_avg.txt.  Mode 2 is held bit for bit
against the torch expression m += (x - m) / (k + 1) run on the GPU (what utils/precise_bn.py computed per layer).

The bad-device-row case enlarges a numel across a chunk boundary: that is what a workgroup can tell from the chunk
list (an enlargement inside the last chunk's slack looks like a valid table)."""
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

pytestmark = pytest.mark.gpu
MARGIN, SENTINEL, WORD_SENTINEL = 256, -777.0, -777
UPDATES = 4
BUFFERS = (3, 5)  # the tensors that are float BUFFERS of the module (copied with use_buffers=False): sizes 4 and C - 1
_REF = {}


def _wa():
    from slowfast.models import weight_avg
    return weight_avg


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _numels():
    C = _chunk()
    return [C, 1, 3, 4, 5, C - 1, C + 1, 2 * C + 1]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _guarded(n, dtype=torch.float32):
    """A buffer of n elements between two sentinel margins -> (whole allocation, the buffer)."""
    whole = torch.full((MARGIN + n + MARGIN,), SENTINEL if dtype == torch.float32 else WORD_SENTINEL, dtype=dtype,
                       device="cuda")
    return whole, whole[MARGIN:MARGIN + n]


def _margins_intact(whole):
    s = SENTINEL if whole.dtype == torch.float32 else WORD_SENTINEL
    return bool((whole[:MARGIN] == s).all()) and bool((whole[-MARGIN:] == s).all())


def _snapshots():
    """UPDATES source states: eight float tensors and the word, seeded."""
    g = torch.Generator().manual_seed(0)
    return [([torch.randn(n, generator=g) for n in _numels()], 5 + k) for k in range(UPDATES)]


class _Side(object):
    """One side of the pairs: the eight float tensors as views of ONE guarded flat buffer (packed tightly, or every
    view on 16 bytes with `aligned`) and the word in a guarded int64 buffer."""

    def __init__(self, aligned=False):
        numels = _numels()
        offs, n = [], 0
        for k in numels:
            offs.append(n)
            n += (k + 3) // 4 * 4 if aligned else k
        self.whole, flat = _guarded(n)
        flat.fill_(float("nan"))
        assert flat.data_ptr() % 16 == 0
        self.views = [flat[o:o + k] for o, k in zip(offs, numels)]
        self.whole_w, self.word = _guarded(1, torch.int64)
        assert self.word.data_ptr() % 8 == 0

    def load(self, snap):
        for v, t in zip(self.views, snap[0]):
            v.copy_(t)
        self.word.fill_(snap[1])

    def clone(self):
        return [v.clone() for v in self.views], self.word.clone()

    def intact(self):
        return _margins_intact(self.whole) and _margins_intact(self.whole_w)


def _tables(avg, src, kinds):
    wa = _wa()
    entries = [(a.data_ptr(), s.data_ptr(), a.numel(), k) for a, s, k in zip(avg.views, src.views, kinds)]
    entries.append((avg.word.data_ptr(), src.word.data_ptr(), 1, wa.KIND_WORDS))
    table, chunks = wa.build_avg_tables(entries, _chunk())
    return table, table.cuda(), chunks, chunks.cuda()


def _kinds(copied=BUFFERS):
    return [1 if i in copied else 0 for i in range(8)]


class _Bag(torch.nn.Module):
    def __init__(self, snap, dtype, device):
        super().__init__()
        for i, t in enumerate(snap[0]):
            t = t.to(device=device, dtype=dtype)
            if i in BUFFERS:
                self.register_buffer("t%d" % i, t.clone())
            else:
                setattr(self, "t%d" % i, torch.nn.Parameter(t.clone()))
        self.register_buffer("num", torch.tensor(snap[1], dtype=torch.int64, device=device))

    def load(self, snap):
        with torch.no_grad():
            for i, t in enumerate(snap[0]):
                getattr(self, "t%d" % i).copy_(t)
            self.num.fill_(snap[1])


def _torch_run(decay, device, dtype):
    """torch's AveragedModel(use_buffers=False) over the snapshots -> per update, the eight averaged tensors (float64,
    on the CPU)."""
    key = (decay, device, dtype)
    if key not in _REF:
        snaps = _snapshots()
        bag = _Bag(snaps[0], dtype, device)
        kw = {} if decay is None else {"multi_avg_fn": get_ema_multi_avg_fn(decay)}
        avg = AveragedModel(bag, use_buffers=False, **kw)
        out = []
        for snap in snaps:
            bag.load(snap)
            avg.update_parameters(bag)
            out.append([getattr(avg.module, "t%d" % i).detach().double().cpu().clone() for i in range(8)])
        assert int(avg.n_averaged) == UPDATES
        _REF[key] = out
    return _REF[key]


def _hip_run(decay, aligned=False):
    """The same updates through sf_avg_update -> (per update: averaged tensors, word), the sides, the count."""
    wa = _wa()
    avg, src = _Side(aligned), _Side(aligned)
    tabs = _tables(avg, src, _kinds())
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    mode, hyper_host, hyper = wa.MODE_MEAN, None, None
    if decay is not None:
        mode, hyper_host = wa.MODE_EMA, torch.tensor([1.0 - decay], dtype=torch.float32)
        hyper = hyper_host.cuda()
    out = []
    for snap in _snapshots():
        src.load(snap)
        wa.avg_update(*tabs, mode, count, hyper_host=hyper_host, hyper=hyper)
        out.append(avg.clone())
    torch.cuda.synchronize()
    return out, avg, src, count


@pytest.mark.parametrize("decay", [0.999, 0.5, 0.25, None])
def test_ema_and_swa_match_float64_within_twice_torchs_own_error(decay):
    """decays 0.999 / 0.5 / 0.25: the weights 0.001, 0.5, 0.75 take both branches of torch's lerp; None: mode 1."""
    ref = _torch_run(decay, "cpu", torch.float64)
    own = _torch_run(decay, "cuda", torch.float32)
    got, avg, src, count = _hip_run(decay)
    al = [v.data_ptr() % 16 for v in avg.views]
    assert 0 in al and any(a in (4, 8, 12) for a in al)  # 16-byte aligned and merely 4-byte aligned views
    snaps = _snapshots()
    for k in range(UPDATES):
        e = t = 0.0
        for i in range(8):
            if i in BUFFERS:
                continue
            e = max(e, float((got[k][0][i].double().cpu() - ref[k][i]).abs().max()))
            t = max(t, float((own[k][i] - ref[k][i]).abs().max()))
        print("decay %s update %d: averaged-parameter err %.3e (torch's float32 foreach run %.3e)" % (decay, k + 1, e, t))
        assert e <= 2 * t, (k, e, t)
        # kinds 1 and 2: the source, exactly, after every update
        for i in BUFFERS:
            assert _same_bits(got[k][0][i].cpu(), snaps[k][0][i]), (k, i)
        assert int(got[k][1]) == snaps[k][1]
    for i in range(8):  # the first update is a copy
        assert _same_bits(got[0][0][i].cpu(), snaps[0][0][i]), i
    assert int(count) == UPDATES
    assert avg.intact() and src.intact()
    assert all(_same_bits(v.cpu(), t) for v, t in zip(src.views, snaps[-1][0]))  # the sources are only read


def test_running_mean_mode_equals_the_torch_expression_bit_for_bit():
    wa = _wa()
    avg, src = _Side(), _Side()
    tabs = _tables(avg, src, [0] * 8)
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    want = [torch.zeros(n, device="cuda") for n in _numels()]
    for k, snap in enumerate(_snapshots()):
        src.load(snap)
        wa.avg_update(*tabs, wa.MODE_RUNNING, count)
        for m, x in zip(want, src.views):
            m += (x - m) / (k + 1)
        for i, (a, m) in enumerate(zip(avg.views, want)):
            assert _same_bits(a, m), (k, i)
        assert int(avg.word) == snap[1]
    assert int(count) == UPDATES and avg.intact() and src.intact()


@pytest.mark.parametrize("value", [1.0, float("nan")])
def test_a_raised_guard_moves_nothing(value):
    wa = _wa()
    snaps = _snapshots()
    avg, src = _Side(), _Side()
    tabs = _tables(avg, src, _kinds())
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    hyper_host = torch.tensor([0.25], dtype=torch.float32)
    hyper = hyper_host.cuda()
    low = torch.zeros(1, device="cuda")
    for snap in snaps[:2]:
        src.load(snap)
        wa.avg_update(*tabs, wa.MODE_EMA, count, hyper_host=hyper_host, hyper=hyper, guard=low)  # a guard at rest
    before, before_w = avg.clone()
    assert int(count) == 2 and not any(bool(torch.isnan(v).any()) for v in before)
    src.load(snaps[2])
    guard = torch.full((1,), value, device="cuda")
    for mode in (wa.MODE_EMA, wa.MODE_MEAN, wa.MODE_RUNNING):
        wa.avg_update(*tabs, mode, count, hyper_host=hyper_host, hyper=hyper, guard=guard)
    torch.cuda.synchronize()
    assert int(count) == 2
    assert all(_same_bits(a, b) for a, b in zip(avg.views, before)) and int(avg.word) == int(before_w)
    assert avg.intact() and src.intact()
    wa.avg_update(*tabs, wa.MODE_EMA, count, hyper_host=hyper_host, hyper=hyper, guard=low)
    assert int(count) == 3 and not _same_bits(avg.views[0], before[0])


@pytest.mark.parametrize("row,numel", [(4, "5 + 2 C"), (6, "3 C + 5"), (7, "C")])
def test_a_device_row_that_differs_from_the_checked_host_copy_writes_nothing(row, numel):
    """The device table's numel of one tensor grew (or shrank) across a chunk boundary behind the host's check: every
    chunk of that tensor is switched off, the other tensors are updated as usual, nothing lands outside a tensor."""
    wa = _wa()
    C = _chunk()
    snaps = _snapshots()
    avg, src = _Side(), _Side()
    table, table_dev, chunks, chunks_dev = _tables(avg, src, [0] * 8)
    bad = table.clone()
    bad[row, 2] = {"5 + 2 C": 5 + 2 * C, "3 C + 5": 3 * C + 5, "C": C}[numel]
    bad_dev = bad.cuda()
    count = torch.zeros((), dtype=torch.int64, device="cuda")
    src.load(snaps[0])
    marker = [torch.full_like(v, 3.25) for v in avg.views]
    for v, m in zip(avg.views, marker):
        v.copy_(m)
    wa.avg_update(table, bad_dev, chunks, chunks_dev, wa.MODE_MEAN, count)
    torch.cuda.synchronize()
    for i in range(8):
        assert _same_bits(avg.views[i], marker[i] if i == row else src.views[i]), i
    assert avg.intact() and src.intact() and int(count) == 1
    wa.avg_exchange(table, bad_dev, chunks, chunks_dev, wa.OP_SWAP)
    torch.cuda.synchronize()
    assert _same_bits(avg.views[row], marker[row]) and _same_bits(src.views[row].cpu(), snaps[0][0][row])
    assert avg.intact() and src.intact()


def test_exchange_swaps_exactly_and_twice_restores_every_bit():
    wa = _wa()
    snaps = _snapshots()
    avg, src = _Side(), _Side()
    tabs = _tables(avg, src, _kinds())
    avg.load(snaps[0])
    src.load(snaps[1])
    avg.views[2][1] = float("nan")  # a NaN payload and a negative zero travel as bits
    avg.views[2][2] = -0.0
    a0, a0w = avg.clone()
    s0, s0w = src.clone()
    wa.avg_exchange(*tabs, wa.OP_SWAP)
    torch.cuda.synchronize()
    assert all(_same_bits(a, s) for a, s in zip(avg.views, s0)) and all(_same_bits(s, a) for s, a in zip(src.views, a0))
    assert int(avg.word) == int(s0w) and int(src.word) == int(a0w)
    assert avg.intact() and src.intact()
    wa.avg_exchange(*tabs, wa.OP_SWAP)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(avg.views, a0)) and all(_same_bits(s, b) for s, b in zip(src.views, s0))
    assert int(avg.word) == int(a0w) and int(src.word) == int(s0w)
    assert avg.intact() and src.intact()


def test_exchange_copies_one_way():
    wa = _wa()
    snaps = _snapshots()
    avg, src = _Side(), _Side()
    tabs = _tables(avg, src, _kinds())
    avg.load(snaps[0])
    src.load(snaps[1])
    a0, a0w = avg.clone()
    wa.avg_exchange(*tabs, wa.OP_TO_SOURCE)  # average -> source
    torch.cuda.synchronize()
    assert all(_same_bits(s, a) for s, a in zip(src.views, a0)) and all(_same_bits(a, b) for a, b in zip(avg.views, a0))
    assert int(src.word) == int(a0w) == int(avg.word) and avg.intact() and src.intact()
    src.load(snaps[2])
    s0, s0w = src.clone()
    wa.avg_exchange(*tabs, wa.OP_FROM_SOURCE)  # source -> average
    torch.cuda.synchronize()
    assert all(_same_bits(a, s) for a, s in zip(avg.views, s0)) and all(_same_bits(s, b) for s, b in zip(src.views, s0))
    assert int(avg.word) == int(s0w) == int(src.word) and avg.intact() and src.intact()


def test_aligned_and_unaligned_views_give_identical_bits():
    wa = _wa()
    for decay in (0.999, 0.25, None):
        packed, _, _, _ = _hip_run(decay)
        aligned, avg, _, _ = _hip_run(decay, aligned=True)
        assert all(v.data_ptr() % 16 == 0 for v in avg.views)
        for k in range(UPDATES):
            assert all(_same_bits(a, b) for a, b in zip(packed[k][0], aligned[k][0])), (decay, k)
    results = []
    for aligned in (False, True):
        avg, src = _Side(aligned), _Side(aligned)
        tabs = _tables(avg, src, [0] * 8)
        count = torch.zeros((), dtype=torch.int64, device="cuda")
        for snap in _snapshots():
            src.load(snap)
            wa.avg_update(*tabs, wa.MODE_RUNNING, count)
        wa.avg_exchange(*tabs, wa.OP_SWAP)
        torch.cuda.synchronize()
        results.append((avg.clone()[0], src.clone()[0]))
        assert avg.intact() and src.intact()
    for side in (0, 1):
        assert all(_same_bits(a, b) for a, b in zip(results[0][side], results[1][side]))
