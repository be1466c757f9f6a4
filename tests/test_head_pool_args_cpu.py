"""Argument checks of the fully-convolutional head's pooling entries (sf_avgpool_win_fwd / sf_avgpool_win_bwd) run
without a GPU: every call below must be refused with SF_EINVAL before any launch, so no call here passes a valid
argument set and the host memory behind the pointers is never touched."""
import ctypes

_buf = (ctypes.c_float * 64)()
_base = ctypes.addressof(_buf)
_base += (-_base) % 16
P = ctypes.c_void_p(_base)  # 16-byte aligned


def _lib():
    import os
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def _desc(**kw):
    """N2 T2 H4 W4 C8 under a (2,2,2) window: the head's case, valid until `kw` breaks it."""
    import sfhip
    f = dict(N=2, Ti=2, Hi=4, Wi=4, C=8, in_cs=16, in_coff=4, To=1, Ho=3, Wo=3, out_cs=24, out_coff=8,
             kT=2, kH=2, kW=2, sT=1, sH=1, sW=1, pT=0, pH=0, pW=0, is_avg=1)
    f.update(kw)
    return sfhip.PoolDesc(*[f[n] for n, _ in sfhip.PoolDesc._fields_])


def _fwd(L, d, x=P, out=P):
    return L.sf_avgpool_win_fwd(ctypes.byref(d) if d is not None else None, x, out, None)


def _bwd(L, d, dy=P, dy_cs=24, dy_coff=8, dx=P, dx_cs=16, dx_coff=4, overwrite=1):
    return L.sf_avgpool_win_bwd(ctypes.byref(d) if d is not None else None, dy, dy_cs, dy_coff, dx, dx_cs, dx_coff,
                                overwrite, None)


def test_null_pointers_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    assert _fwd(L, None) == E and _fwd(L, _desc(), x=None) == E and _fwd(L, _desc(), out=None) == E
    assert _bwd(L, None) == E and _bwd(L, _desc(), dy=None) == E and _bwd(L, _desc(), dx=None) == E


def test_non_positive_dims_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for name in ("N", "Ti", "Hi", "Wi", "C", "kT", "kH", "kW"):
        for bad in (0, -1):
            d = _desc(**{name: bad})
            assert _fwd(L, d) == E and _bwd(L, d) == E, (name, bad)


def test_window_larger_than_the_input_is_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(kT=3, To=0), dict(kH=5, Ho=0), dict(kW=5, Wo=0), dict(kT=3, To=1), dict(kH=5, Ho=1)):
        d = _desc(**kw)
        assert _fwd(L, d) == E and _bwd(L, d) == E, kw


def test_anything_but_a_stride_1_unpadded_average_is_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(sH=2), dict(sT=0), dict(pW=1), dict(is_avg=0), dict(Ho=2), dict(To=2), dict(Wo=4)):
        d = _desc(**kw)
        assert _fwd(L, d) == E and _bwd(L, d) == E, kw


def test_channel_slices_outside_their_pitch_are_refused():
    import sfhip
    L, E = _lib(), sfhip.SF_EINVAL
    for kw in (dict(in_coff=12), dict(in_coff=-4), dict(out_coff=20), dict(out_cs=4), dict(in_cs=0)):
        assert _fwd(L, _desc(**kw)) == E, kw
    for kw in (dict(dy_coff=20), dict(dy_coff=-4), dict(dx_coff=12), dict(dx_cs=4), dict(dy_cs=0)):
        assert _bwd(L, _desc(), **kw) == E, kw
