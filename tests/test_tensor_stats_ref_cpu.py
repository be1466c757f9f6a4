"""tests/_tensor_stats_ref.py (the numpy restatement of sf_tensor_stats' row) held to rows worked out by hand: every bin
edge, the clamps at both ends, denormals and zeros in the centre bin, non-finite elements in no bin, and the identity
sum(hist) + n_nan + n_inf == numel."""
import numpy as np

import _tensor_stats_ref as ref

B = ref.B
f32 = np.float32
LO = f32(2.0 ** -20)


def test_bin_edges_by_hand():
    # bins: [0 .. B-1] negative, largest magnitude first; [B] centre; [B+1 .. 2B] positive, smallest magnitude first
    assert ref.N_HIST == 49 and B == 24
    below, above = np.nextafter(LO, f32(0.0)), np.nextafter(LO, f32(1.0))
    assert below < LO < above
    by_hand = [
        (LO, B + 1), (above, B + 1), (below, B),                     # 2^-20 opens the first positive bin
        (-LO, B - 1), (-above, B - 1), (-below, B),                  # ... and -2^-20 the first negative one
        (f32(2.0 ** -19), B + 2), (np.nextafter(f32(2.0 ** -19), f32(0.0)), B + 1),
        (f32(1.0), B + 21), (f32(-1.0), B - 21), (f32(1.5), B + 21), (f32(2.0), B + 22), (f32(4.0), B + 23),
        (np.nextafter(f32(8.0), f32(0.0)), B + 23),                  # [2^2, 2^3) is bin k = 22
        (f32(8.0), 2 * B), (f32(16.0), 2 * B), (np.finfo(f32).max, 2 * B),   # k = 23: everything at or above 2^3
        (f32(-8.0), 0), (f32(-16.0), 0), (-np.finfo(f32).max, 0),
        (np.finfo(f32).tiny, B), (f32(1e-40), B), (f32(-1e-40), B), (f32(0.0), B), (f32(-0.0), B),
    ]
    for x, want in by_hand:
        assert ref.bin_of(x) == want, (x, ref.bin_of(x), want)
        assert ref.ref_row(np.array([x], dtype=f32)).hist[want] == 1, x


def test_a_row_by_hand():
    x = np.array([0.0, -0.0, 1.0, -2.0, 3.0, np.nan, np.inf, -np.inf, 1e-40, 2.0 ** -20, 16.0, np.nan], dtype=f32)
    r = ref.ref_row(x)
    assert (r.present, r.numel, r.n_nan, r.n_inf, r.n_zero) == (1, 12, 2, 2, 2)
    assert (r.min, r.max, r.absmax) == (f32(-2.0), f32(16.0), f32(16.0))
    small = float(f32(1e-40)) + 2.0 ** -20
    assert r.sum == 18.0 + small and abs(r.sumsq - (1.0 + 4.0 + 9.0 + 256.0 + 2.0 ** -40)) < 1e-12
    hist = [0] * 49
    hist[B] = 3                    # +0, -0, the denormal
    hist[B + 21] = 1               # 1.0: e = 0
    hist[B - 22] = 1               # -2.0: e = 1
    hist[B + 22] = 1               # 3.0: e = 1
    hist[B + 1] = 1                # 2^-20
    hist[2 * B] = 1                # 16.0, clamped
    assert list(r.hist) == hist
    assert sum(r.hist) + r.n_nan + r.n_inf == r.numel


def test_no_finite_element_and_the_absent_row():
    r = ref.ref_row(np.array([np.nan, np.inf], dtype=f32))
    assert (r.n_nan, r.n_inf, r.n_zero, sum(r.hist)) == (1, 1, 0, 0)
    assert r.min == f32(np.inf) and r.max == f32(-np.inf) and r.absmax == f32(0.0)
    assert r.sum == 0.0 and r.sumsq == 0.0
    a = ref.ABSENT
    assert a.present == 0 and a.numel == 0 and sum(a.hist) == 0 and a.sum == 0.0


def test_identity_and_edges_on_seeded_data():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(5000) * np.exp2(rng.uniform(-30, 10, 5000))).astype(f32)
    edges = ref.edge_values()
    assert edges.size == 13 and np.isfinite(edges).all()
    x[:edges.size] = edges
    x[100], x[200], x[300] = np.nan, np.inf, -np.inf
    r = ref.ref_row(x)
    assert sum(r.hist) + r.n_nan + r.n_inf == r.numel == 5000
    assert (r.n_nan, r.n_inf) == (1, 2) and r.n_zero == 2
    assert list(r.hist) == np.bincount([ref.bin_of(v) for v in x if np.isfinite(v)], minlength=49).tolist()
    assert min(r.hist) > 0  # the generator reaches every bin
