"""Argument checks of the memory-bound entry points (sf_affine_fwd / _split / _mask, sf_row_softmax_fwd / _bwd,
sf_sigmoid_bwd, sf_pool_fwd) run without a GPU: every call below must be refused before any launch, so no call here
passes a valid argument set and the host memory behind the pointers is never touched."""
import ctypes


def _lib():
    import sfhip
    import os
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned


def _affine(L, x=P, cs=20, coff=4, N=3, T=2, H=5, W=7, C=12, scale=P, bias=P, res=None, res_cs=0, res_coff=0, act=1,
            rep=1, out=P, out_cs=24, out_coff=8, out_cmul=1, nsplit=None):
    head = (x, cs, coff, N, T, H, W, C)
    tail = (scale, bias, res, res_cs, res_coff, act, rep, out, out_cs, out_coff, out_cmul, None)
    if nsplit is None:
        return L.sf_affine_fwd(*(head + tail))
    return L.sf_affine_fwd_split(*(head + (nsplit,) + tail))


def _affine_mask(L, x=P, cs=20, coff=4, C=12, scale=P, bias=P, act=1, out=P, out_cs=24, out_coff=8, mask=P):
    return L.sf_affine_fwd_mask(x, cs, coff, 3, 2, 5, 7, C, scale, bias, None, 0, 0, act, out, out_cs, out_coff, mask,
                                None)


def test_affine_entries_refuse_bad_arguments():
    import sfhip
    L = _lib()
    E = sfhip.SF_EINVAL
    assert _affine(L, bias=None) == E and _affine(L, scale=None) == E  # one of the pair without the other
    assert _affine(L, rep=0) == E and _affine(L, rep=-1) == E
    assert _affine(L, out_cmul=0) == E
    assert _affine(L, act=sfhip.ACT_SIGMOID) == E and _affine(L, act=7) == E and _affine(L, act=-1) == E
    assert _affine(L, x=None) == E and _affine(L, out=None) == E
    for dim in ("N", "T", "H", "W", "C"):
        assert _affine(L, **{dim: 0}) == E, dim
    assert _affine(L, nsplit=0) == E and _affine(L, nsplit=-2) == E
    assert _affine(L, nsplit=2, rep=0) == E and _affine(L, nsplit=2, x=None) == E


def test_affine_mask_entry_refuses_what_the_flat_kernel_cannot_take():
    import sfhip
    L = _lib()
    E = sfhip.SF_EINVAL
    assert _affine_mask(L, act=sfhip.ACT_NONE) == E
    assert _affine_mask(L, mask=None) == E
    assert _affine_mask(L, C=7) == E             # no float4 channels
    assert _affine_mask(L, out_coff=2) == E      # the output slice is not 16-byte addressable
    assert _affine_mask(L, coff=3) == E and _affine_mask(L, cs=22) == E
    assert _affine_mask(L, x=None) == E and _affine_mask(L, out=None) == E
    assert _affine_mask(L, bias=None) == E


def test_row_softmax_entries_refuse_bad_arguments():
    import sfhip
    L = _lib()
    E = sfhip.SF_EINVAL
    assert L.sf_row_softmax_fwd(None, 23, 3, 18, 18, 1.0, None) == E
    assert L.sf_row_softmax_fwd(P, 23, 3, 0, 18, 1.0, None) == E
    assert L.sf_row_softmax_fwd(P, 23, 3, -4, 18, 1.0, None) == E
    assert L.sf_row_softmax_fwd(P, 23, 3, 18, 0, 1.0, None) == E
    assert L.sf_row_softmax_fwd(P, 23, 3, 18, -1, 1.0, None) == E
    assert L.sf_row_softmax_bwd(None, 23, 3, P, 26, 4, 18, 18, 1.0, None) == E
    assert L.sf_row_softmax_bwd(P, 23, 3, None, 26, 4, 18, 18, 1.0, None) == E
    assert L.sf_row_softmax_bwd(P, 23, 3, P, 26, 4, 0, 18, 1.0, None) == E
    assert L.sf_row_softmax_bwd(P, 23, 3, P, 26, 4, -1, 18, 1.0, None) == E
    assert L.sf_row_softmax_bwd(P, 23, 3, P, 26, 4, 18, 0, 1.0, None) == E


def test_sigmoid_bwd_entry_refuses_bad_arguments_and_accepts_nothing_to_do():
    import sfhip
    L = _lib()
    E = sfhip.SF_EINVAL
    assert L.sf_sigmoid_bwd(None, P, P, 400, 1, None) == E
    assert L.sf_sigmoid_bwd(P, None, P, 400, 1, None) == E
    assert L.sf_sigmoid_bwd(P, P, None, 400, 0, None) == E
    assert L.sf_sigmoid_bwd(P, P, P, -1, 1, None) == E
    assert L.sf_sigmoid_bwd(P, P, P, 0, 1, None) == 0       # SF_OK: no element, no launch
    assert L.sf_sigmoid_bwd(None, None, None, 0, 0, None) == 0


def test_pool_entry_refuses_bad_arguments():
    import sfhip
    L = _lib()
    E = sfhip.SF_EINVAL

    def desc(**kw):
        f = dict(N=2, Ti=4, Hi=13, Wi=12, C=8, in_cs=20, in_coff=4, To=4, Ho=7, Wo=6, out_cs=16, out_coff=4,
                 kT=3, kH=3, kW=3, sT=1, sH=2, sW=2, pT=1, pH=1, pW=1, is_avg=0)
        f.update(kw)
        return sfhip.PoolDesc(*[f[n] for n, _ in sfhip.PoolDesc._fields_])

    good = desc()
    assert L.sf_pool_fwd(None, P, P, None) == E
    assert L.sf_pool_fwd(ctypes.byref(good), None, P, None) == E
    assert L.sf_pool_fwd(ctypes.byref(good), P, None, None) == E
    for name in ("C", "kT", "kH", "kW", "N", "To", "Ho", "Wo"):
        for bad in (0, -1):
            assert L.sf_pool_fwd(ctypes.byref(desc(**{name: bad})), P, P, None) == E, (name, bad)
