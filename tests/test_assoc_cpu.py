"""Host side of the associative "dot_product" entries (sf_assoc_accepts, sf_gram*, sf_rowmat; attn_assoc.hip): the shape
query, the chunk plan, the workspace query and the argument checks run without a GPU, and the algebra the route in
nonlocal_helper.dense_attention relies on is pinned in fp64 torch."""
import ctypes

import torch


def _lib():
    import sfhip
    import os
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def test_assoc_accepts_is_host_only():
    L = _lib()
    for shape in ((6272, 1568, 256, 256), (1568, 392, 512, 512), (50, 1, 20, 36), (1, 1, 4, 4)):
        assert L.sf_assoc_accepts(*shape) == 1, shape
    for bad in (516, 18, 0, 6):
        assert L.sf_assoc_accepts(64, 64, bad, 64) == 0, bad
        assert L.sf_assoc_accepts(64, 64, 64, bad) == 0, bad
    assert L.sf_assoc_accepts(0, 64, 64, 64) == 0 and L.sf_assoc_accepts(64, 0, 64, 64) == 0


def test_gram_workspace_exists_exactly_where_the_rows_are_split():
    L = _lib()
    seen = set()
    for B in (1, 2, 8):
        for R in (1, 33, 150, 392, 1568, 3000, 6272, 25088):
            for da, db in ((4, 4), (16, 16), (20, 36), (64, 64), (132, 4), (128, 128), (256, 256), (512, 512)):
                S, n = L.sf_gram_splits(B, R, da, db), L.sf_gram_ws_floats(B, R, da, db)
                assert S >= 1
                assert (n == 0) == (S == 1), (B, R, da, db, S, n)
                if S > 1:
                    assert n == S * B * da * db
                assert S == L.sf_gram_splits(1, R, da, db)  # the plan does not depend on the batch
                seen.add(S > 1)
    assert seen == {False, True}


def test_gram_workspace_and_M_are_far_below_one_score_matrix():
    """The backward's D = theta^T dY at the NLN res3 / res4 shapes (R = N_q, N_k = N_q / 4 after the (1,2,2) pool):
    workspace plus one sample's d x dv matrix against one sample's N_q x N_k scores."""
    L = _lib()
    for B, R, da, db in ((8, 6272, 256, 256), (8, 1568, 512, 512)):
        assert L.sf_gram_ws_floats(B, R, da, db) + da * db < R * (R // 4), (B, R, da, db)


def test_assoc_entries_refuse_bad_arguments_without_a_gpu_call():
    import sfhip
    L = _lib()
    # host memory is never touched by the checks
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def gram(a=p, a_cs=20, b=p, b_cs=20, g=p, gt=p, B=1, R=8, da=16, db=20, ws=p):
        return L.sf_gram(a, a_cs, b, b_cs, g, gt, B, R, da, db, 1.0, ws, None)

    def rowmat(x=p, x_cs=20, w=p, y=p, y_cs=20, B=1, R=8, k=16, n=20):
        return L.sf_rowmat(x, x_cs, w, y, y_cs, B, R, k, n, 1.0, 0, None)

    assert gram(a=None) == sfhip.SF_EINVAL and gram(b=None) == sfhip.SF_EINVAL and gram(g=None) == sfhip.SF_EINVAL
    assert gram(a=off) == sfhip.SF_EALIGN and gram(b=off) == sfhip.SF_EALIGN
    assert gram(g=off) == sfhip.SF_EALIGN and gram(gt=off) == sfhip.SF_EALIGN
    assert gram(a_cs=18) == sfhip.SF_EALIGN and gram(b_cs=22) == sfhip.SF_EALIGN
    assert gram(a_cs=12) == sfhip.SF_EINVAL and gram(b_cs=16) == sfhip.SF_EINVAL
    assert gram(B=0) == sfhip.SF_EINVAL and gram(R=0) == sfhip.SF_EINVAL
    assert gram(da=18) == sfhip.SF_ENOTTAKEN and gram(db=516, b_cs=516) == sfhip.SF_ENOTTAKEN
    assert L.sf_gram_splits(1, 3000, 16, 16) > 1
    assert gram(R=3000, ws=None) == sfhip.SF_EINVAL  # a split shape without its workspace

    assert rowmat(x=None) == sfhip.SF_EINVAL and rowmat(w=None) == sfhip.SF_EINVAL and rowmat(y=None) == sfhip.SF_EINVAL
    assert rowmat(x=off) == sfhip.SF_EALIGN and rowmat(w=off) == sfhip.SF_EALIGN and rowmat(y=off) == sfhip.SF_EALIGN
    assert rowmat(x_cs=18) == sfhip.SF_EALIGN and rowmat(y_cs=22) == sfhip.SF_EALIGN
    assert rowmat(x_cs=12) == sfhip.SF_EINVAL and rowmat(y_cs=16) == sfhip.SF_EINVAL
    assert rowmat(B=0) == sfhip.SF_EINVAL and rowmat(R=0) == sfhip.SF_EINVAL
    assert rowmat(k=18) == sfhip.SF_ENOTTAKEN and rowmat(n=516, y_cs=516) == sfhip.SF_ENOTTAKEN


def test_associative_products_equal_autograd_through_the_scores():
    """Forward Y = theta (phi^T g / N_k) and the backward's D = theta^T dY, dtheta = dY M^T, dg = phi D / N_k,
    dphi = g D^T / N_k — written with gram(a, b) = a^T b and rowmat(x, w) = x w^T exactly as dense_attention calls
    them — against fp64 autograd through (theta phi^T / N_k) g."""
    gen = torch.Generator().manual_seed(11)
    B, nq, nk, d, dv = 2, 37, 13, 20, 36
    theta, phi, g, dy = [torch.randn(s, generator=gen, dtype=torch.float64)
                         for s in ((B, nq, d), (B, nk, d), (B, nk, dv), (B, nq, dv))]
    t, p, v = [x.clone().requires_grad_(True) for x in (theta, phi, g)]
    y_ref = ((t @ p.transpose(1, 2)) / nk) @ v
    y_ref.backward(dy)

    def gram(a, b, alpha):
        G = alpha * (a.transpose(1, 2) @ b)
        return G, G.transpose(1, 2).contiguous()

    def rowmat(x, w, alpha):
        return alpha * (x @ w.transpose(1, 2))

    Mt, M = gram(g, phi, 1.0 / nk)
    assert Mt.shape == (B, dv, d) and M.shape == (B, d, dv)
    y = rowmat(theta, Mt, 1.0)
    D, Dt = gram(theta, dy, 1.0)
    dth, dg, dph = rowmat(dy, M, 1.0), rowmat(phi, Dt, 1.0 / nk), rowmat(g, D, 1.0 / nk)
    for name, a, b in (("y", y, y_ref.detach()), ("dtheta", dth, t.grad), ("dphi", dph, p.grad), ("dg", dg, v.grad)):
        assert a.shape == b.shape, name
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, name
