"""Host side of the streaming cross-length attention entries (sf_xattn_*, attn_cross.hip): the shape query, the
workspace query and the argument checks run without a GPU."""
import ctypes


def _lib():
    import sfhip
    import os
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def test_xattn_accepts_is_host_only():
    L = _lib()
    for shape in ((6272, 1568, 256, 256), (1568, 392, 512, 512), (50, 1, 20, 36), (1, 1, 4, 4), (40, 200, 132, 4)):
        assert L.sf_xattn_accepts(*shape) == 1, shape
    for shape in ((64, 64, 516, 64), (64, 64, 18, 64), (64, 64, 64, 0), (64, 0, 64, 64), (0, 64, 64, 64),
                  (64, 64, 64, 516), (64, 64, 0, 64), (64, 64, 64, 6)):
        assert L.sf_xattn_accepts(*shape) == 0, shape


def test_xattn_backward_workspace_is_far_below_the_score_matrix():
    L = _lib()
    for B, nq, nk, d, dv in ((8, 6272, 1568, 256, 256), (8, 1568, 392, 512, 512), (2, 50, 1, 20, 36)):
        assert L.sf_xattn_bwd_ws_floats(B, nq, nk, d, dv) >= 0
    assert L.sf_xattn_bwd_ws_floats(1, 6272, 1568, 256, 256) < 6272 * 1568 / 4
    assert L.sf_xattn_bwd_ws_floats(8, 6272, 1568, 256, 256) < 6272 * 1568 / 4


def test_xattn_entries_refuse_bad_arguments_without_a_gpu_call():
    import sfhip
    L = _lib()
    rc = L.sf_xattn_fwd(None, 256, None, 256, None, 256, None, 256, None, 2, 64, 32, 256, 256, 1.0, None)
    assert rc < 0
    rc = L.sf_xattn_bwd(None, 64, None, 64, None, 64, None, 64, None, None, None, 64, None, 64, None, 64, 0, 2, 64, 32,
                        64, 64, 1.0, None, None)
    assert rc < 0
    # host memory is never touched by the checks: a refused shape, a misaligned view and a pitch below the width
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    assert L.sf_xattn_fwd(p, 20, p, 20, p, 20, p, 20, p, 1, 8, 8, 18, 20, 1.0, None) == sfhip.SF_ENOTTAKEN
    assert L.sf_xattn_fwd(off, 20, p, 20, p, 20, p, 20, p, 1, 8, 8, 16, 20, 1.0, None) == sfhip.SF_EALIGN
    assert L.sf_xattn_fwd(p, 18, p, 20, p, 20, p, 20, p, 1, 8, 8, 16, 20, 1.0, None) == sfhip.SF_EALIGN
    assert L.sf_xattn_fwd(p, 12, p, 20, p, 20, p, 20, p, 1, 8, 8, 16, 20, 1.0, None) == sfhip.SF_EINVAL
    assert L.sf_xattn_fwd(p, 20, p, 20, p, 20, p, 20, p, 0, 8, 8, 16, 20, 1.0, None) == sfhip.SF_EINVAL
