"""sf_tensor_stats on the GPU (csrc/tensor_stats.hip) through sfhip.tensor_stats and slowfast/utils/model_stats.py, on one
table of tensors of numel 1, 3, 4, 5, 255, C - 1, C, C + 1 and 2 C + 1 (C = sf_sgd_chunk_elems() = 4096: the sub-group
tail, one chunk exactly, the chunk boundary on both sides, three chunks), filled from a seeded generator spanning
2^-30 .. 2^10 with both signs, with planted zeros, a denormal, every bin-edge value of the CPU test and, in two of the
tensors, NaN, +Inf and -Inf.  The reference is tests/_tensor_stats_ref.py: integer fields and min / max / absmax
exactly, sum and sumsq within numel * 2^-52 * sum |term|."""
import numpy as np
import pytest
import torch

import _tensor_stats_ref as ref

pytestmark = pytest.mark.gpu
POISON = 0x5A5A5A5A5A5A5A5A
_DATA = {}


def _chunk():
    import sfhip
    return sfhip.lib().sf_sgd_chunk_elems()


def _data():
    """[(name, float32 numpy array)] and {name: reference Row}, made once and never changed."""
    if not _DATA:
        C = _chunk()
        assert C == 4096
        rng = np.random.default_rng(20260101)
        edges = ref.edge_values()
        arrays = []
        for n in (1, 3, 4, 5, 255, C - 1, C, C + 1, 2 * C + 1):
            x = (rng.standard_normal(n) * np.exp2(rng.uniform(-30, 10, n))).astype(np.float32)
            if n == 4:
                x[:3] = (0.0, -0.0, 1e-40)
            if n >= 255:  # every edge value, spread over the tensor, the last elements (the sub-group tail) included
                pos = np.linspace(0, n - 1, edges.size).astype(np.int64)
                x[pos] = edges
            if n in (5, C + 1):
                x[1:4] = (np.nan, np.inf, -np.inf)
            if n == C + 1:
                x[C - 2], x[C] = -np.inf, np.nan  # on both sides of the chunk boundary (the edge value at C went)
            arrays.append(("t%d" % n, x))
        _DATA["arrays"] = arrays
        _DATA["rows"] = {name: ref.ref_row(x) for name, x in arrays}
        assert sum(r.n_nan + r.n_inf > 0 for r in _DATA["rows"].values()) == 2
    return _DATA["arrays"], _DATA["rows"]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _tables(tensors, absent=()):
    """(table_host, table, chunks_host, chunks) over `tensors`; the rows listed in `absent` get address 0."""
    from slowfast.models.step_tail import build_clip_tables
    entries = [(0 if i in absent else t.data_ptr(), t.numel()) for i, t in enumerate(tensors)]
    table, chunks = build_clip_tables(entries, _chunk())
    return table, table.cuda(), chunks, chunks.cuda()


def _memory(n_tensors, n_chunks, slots):
    import sfhip
    ws = torch.empty((sfhip.lib().sf_tensor_stats_ws_bytes(n_chunks) // 8,), dtype=torch.int64, device="cuda")
    ring = torch.full((slots, n_tensors, sfhip.SF_TSTATS_ROW), POISON, dtype=torch.int64, device="cuda")
    cursor = torch.zeros((2,), dtype=torch.int32, device="cuda")
    return ws, ring, cursor


def _parse(ring, slot):
    from slowfast.utils.model_stats import parse_rows
    return parse_rows(ring[slot].cpu().numpy())


def test_rows_match_the_reference_and_the_inputs_stay():
    from slowfast.utils.model_stats import DeviceModelStats
    arrays, rows = _data()
    tensors = [(name, torch.from_numpy(x).cuda()) for name, x in arrays]
    assert all(t.data_ptr() % 16 == 0 for _, t in tensors)
    watch = DeviceModelStats(tensors, slots=2)
    watch.record("param")
    got = watch.read("param")
    assert len(got) == 1 and list(got[0]) == [name for name, _ in arrays]
    for name, ts in got[0].items():
        print("%-6s n_nan %d n_inf %d n_zero %d min %.6g max %.6g sum err %.3e sumsq err %.3e" % (
            name, ts.n_nan, ts.n_inf, ts.n_zero, ts.min, ts.max, abs(ts.sum - rows[name].sum),
            abs(ts.sumsq - rows[name].sumsq)))
        ref.check_row(ts, rows[name], name)
        n = ts.n_finite
        assert ts.mean == ts.sum / n and ts.rms == (ts.sumsq / n) ** 0.5
    for (name, x), (_, t) in zip(arrays, tensors):
        assert torch.equal(_bits(t).cpu(), _bits(torch.from_numpy(x))), name
    assert watch.cursor("param").tolist() == [1, 1] and watch.cursor("grad").tolist() == [0, 0]
    assert watch.read("grad") == [] and watch.rebuilds == {"param": 1, "grad": 0}


def test_sums_without_a_dominating_element():
    """FLT_MAX among the planted values swallows every other term of sum and sumsq in fp64; the same sizes without the
    planted values hold the two sums to the bound where every term counts."""
    from slowfast.utils.model_stats import DeviceModelStats
    C = _chunk()
    rng = np.random.default_rng(77)
    arrays = [("p%d" % n, (rng.standard_normal(n) * np.exp2(rng.uniform(-30, 10, n))).astype(np.float32))
              for n in (5, 255, C + 1, 2 * C + 1)]
    watch = DeviceModelStats([(name, torch.from_numpy(x).cuda()) for name, x in arrays], slots=1)
    watch.record("param")
    got = watch.read("param")[0]
    for name, x in arrays:
        r = ref.ref_row(x)
        print("%-6s sum %.17g err %.3e, sumsq %.17g err %.3e" % (name, got[name].sum, abs(got[name].sum - r.sum),
                                                                 got[name].sumsq, abs(got[name].sumsq - r.sumsq)))
        ref.check_row(got[name], r, name)


def test_a_misaligned_view_gives_the_aligned_copys_bits_and_two_calls_agree():
    import sfhip
    arrays, rows = _data()
    aligned = [torch.from_numpy(x).cuda() for _, x in arrays]
    shifted = []
    for _, x in arrays:
        big = torch.zeros((x.size + 8,), dtype=torch.float32, device="cuda")
        v = big[1:1 + x.size]  # one float into the buffer: 4-byte aligned only
        v.copy_(torch.from_numpy(x))
        assert v.data_ptr() % 16 == 4
        shifted.append(v)
    out = []
    for tensors in (aligned, shifted):
        tabs = _tables(tensors)
        ws, ring, cursor = _memory(len(tensors), tabs[2].shape[0], 2)
        sfhip.tensor_stats(*tabs, ws, ring, cursor)
        sfhip.tensor_stats(*tabs, ws, ring, cursor)
        torch.cuda.synchronize()
        assert cursor.tolist() == [0, 2]
        assert torch.equal(ring[0], ring[1])  # two calls: bit-identical rows
        out.append(ring[0].clone())
    assert torch.equal(out[0], out[1])
    for (name, _), ts in zip(arrays, _parse(out[1].unsqueeze(0), 0)):
        ref.check_row(ts, rows[name], name)


def test_an_absent_tensor_in_the_middle_gives_a_zero_row():
    import sfhip
    arrays, rows = _data()
    tensors = [torch.from_numpy(x).cuda() for _, x in arrays]
    gone = 7  # the C + 1 tensor: two chunks, so the rows behind it start at a first chunk that is not their index
    tabs = _tables(tensors, absent=(gone,))
    ws, ring, cursor = _memory(len(tensors), tabs[2].shape[0], 1)
    sfhip.tensor_stats(*tabs, ws, ring, cursor)
    torch.cuda.synchronize()
    assert not bool(ring[0, gone].any())  # all zeros, present = 0
    got = _parse(ring, 0)
    assert got[gone].present == 0 and got[gone][:11] == ref.ABSENT[:11]
    for i, (name, _) in enumerate(arrays):
        if i != gone:
            ref.check_row(got[i], rows[name], name)
    assert cursor.tolist() == [0, 1]


def test_the_ring_wraps_and_overwrites_the_oldest_slot_only():
    import sfhip
    arrays, rows = _data()
    tensors = [torch.from_numpy(x).cuda() for _, x in arrays]
    tabs = _tables(tensors)
    ws, ring, cursor = _memory(len(tensors), tabs[2].shape[0], 3)
    for call in range(3):
        tensors[0].fill_(float(call + 1))  # every call sees another t1, so the slots differ
        sfhip.tensor_stats(*tabs, ws, ring, cursor)
    torch.cuda.synchronize()
    assert cursor.tolist() == [0, 3]
    before = ring.clone()
    assert [_parse(ring, s)[0].max for s in range(3)] == [1.0, 2.0, 3.0]
    tensors[0].fill_(4.0)
    sfhip.tensor_stats(*tabs, ws, ring, cursor)
    torch.cuda.synchronize()
    assert cursor.tolist() == [1, 4]  # wrapped
    assert torch.equal(ring[1], before[1]) and torch.equal(ring[2], before[2])  # untouched, bit for bit
    assert not torch.equal(ring[0], before[0])
    got = _parse(ring, 0)
    assert (got[0].min, got[0].max, got[0].sum, got[0].numel) == (4.0, 4.0, 4.0, 1)
    assert torch.equal(ring[0, 1:], before[0, 1:])  # the other tensors did not change
    for i, (name, _) in enumerate(arrays[1:], 1):
        ref.check_row(got[i], rows[name], name)


def test_model_stats_reads_the_ring_oldest_first():
    from slowfast.utils.model_stats import DeviceModelStats
    t = torch.ones((5,), device="cuda")
    watch = DeviceModelStats([("w", t)], slots=3)
    for call in range(5):
        t.fill_(float(call))
        watch.record("param")
    got = watch.read("param")
    assert [g["w"].max for g in got] == [2.0, 3.0, 4.0] and watch.rebuilds["param"] == 1
    assert got[0]["w"].n_zero == 0 and got[0]["w"].hist[ref.bin_of(2.0)] == 5


def test_only_owned_memory_is_written():
    """Workspace, ring and cursor sit inside one poisoned allocation: the call writes the workspace, ONE ring slot and
    the cursor's two words; the other slots, the gaps and the inputs keep their bits."""
    import sfhip
    arrays, rows = _data()
    tensors = [torch.from_numpy(x).cuda() for _, x in arrays]
    tabs = _tables(tensors)
    n, n_chunks, slots, gap = len(tensors), tabs[2].shape[0], 3, 64
    ws_words = sfhip.lib().sf_tensor_stats_ws_bytes(n_chunks) // 8
    ring_words = slots * n * sfhip.SF_TSTATS_ROW
    block = torch.full((4 * gap + ws_words + ring_words + 1,), POISON, dtype=torch.int64, device="cuda")
    o_ws, o_ring = gap, 2 * gap + ws_words
    o_cur = o_ring + ring_words + gap
    ws = block[o_ws:o_ws + ws_words]
    ring = block[o_ring:o_ring + ring_words].view(slots, n, sfhip.SF_TSTATS_ROW)
    cursor = block[o_cur:o_cur + 1].view(torch.int32)
    cursor.copy_(torch.tensor([1, 0], dtype=torch.int32))  # the next slot is 1
    sfhip.tensor_stats(*tabs, ws, ring, cursor)
    torch.cuda.synchronize()
    assert cursor.tolist() == [2, 1]
    for lo, hi in ((0, o_ws), (o_ws + ws_words, o_ring), (o_ring + ring_words, o_cur), (o_cur + 1, block.numel())):
        assert bool((block[lo:hi] == POISON).all()), (lo, hi)
    assert bool((ring[0] == POISON).all()) and bool((ring[2] == POISON).all())
    assert not bool((ring[1] == POISON).any())  # every word of the written slot was written
    for (name, x), ts, t in zip(arrays, _parse(ring, 1), tensors):
        ref.check_row(ts, rows[name], name)
        assert torch.equal(_bits(t).cpu(), _bits(torch.from_numpy(x))), name


def test_grad_tables_follow_addresses_not_identity():
    from slowfast.utils.model_stats import DeviceModelStats, first_bad
    arrays, rows = _data()
    params = [(name, torch.zeros(x.shape, device="cuda").requires_grad_()) for name, x in arrays]
    watch = DeviceModelStats(params, slots=4)
    watch.record("grad")  # no gradient yet: every row absent
    got = watch.read("grad")[0]
    assert all(ts.present == 0 and ts.numel == 0 and sum(ts.hist) == 0 for ts in got.values())
    assert first_bad(got) is None
    flat = torch.cat([torch.from_numpy(x) for _, x in arrays] + [torch.zeros(3)]).cuda()
    off = 0
    for (_, p), (_, x) in zip(params[:-1], arrays):  # the last parameter keeps .grad = None
        p.grad = flat[off:off + x.size].view(x.shape)
        off += x.size
    watch.record("grad")
    assert watch.rebuilds["grad"] == 2
    for (_, p) in params[:-1]:
        p.grad = p.grad.view(-1).view(p.shape)  # another tensor object at the same address
    watch.record("grad")
    assert watch.rebuilds["grad"] == 2  # addresses, not identity
    got = watch.read("grad")
    assert len(got) == 3
    for name, ts in got[2].items():
        if name == arrays[-1][0]:
            assert ts.present == 0
        else:
            ref.check_row(ts, rows[name], name)
    assert first_bad(got[2]) == "t5"
    params[0][1].grad = torch.ones((1,), device="cuda")
    watch.record("grad")
    assert watch.rebuilds["grad"] == 3 and watch.read("grad")[-1]["t1"].max == 1.0
