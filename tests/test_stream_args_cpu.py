"""Every refusal of sf_stream_push / sf_stream_window / sf_label_select is decided on the host before anything is
launched, so it can be asked for without a GPU: the pointers below are never dereferenced on a device."""
import ctypes
import os

import pytest

S, H, W, NEW_H, NEW_W, PH, PW, WP = 8, 20, 28, 16, 22, 3, 3, 30
FAKE = ctypes.c_void_p(4096)  # stands for a 16-byte aligned device pointer


@pytest.fixture(scope="module")
def L():
    import sfhip
    if not os.path.exists(sfhip.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return sfhip.lib()


def test_stream_push_refusals(L):
    import sfhip
    m3 = (ctypes.c_float * 3)(0.45, 0.45, 0.45)
    mp = ctypes.cast(m3, ctypes.c_void_p)

    def call(frame=FAKE, ring=FAKE, mean=mp, std=mp, h=H, w=W, new_h=NEW_H, new_w=NEW_W, s=S, slot=0, ph=PH, pw=PW,
             wp=WP):
        return L.sf_stream_push(frame, h, w, new_h, new_w, mean, std, ring, s, slot, ph, pw, wp, None)

    for kw in (dict(frame=None), dict(ring=None), dict(mean=None), dict(std=None),  # null pointers
               dict(slot=S), dict(slot=-1), dict(slot=S + 5),                      # slot outside [0, S)
               dict(h=0), dict(w=0), dict(new_h=0), dict(new_w=0), dict(new_h=-4), dict(s=0), dict(s=-1),  # sizes
               dict(ph=-1), dict(pw=-1), dict(wp=NEW_W + 2 * PW - 1),              # the row pitch cannot hold a row
               dict(ring=ctypes.c_void_p(4100)),                                   # no 16-byte stores there
               dict(new_h=1 << 20, wp=1 << 12)):                                   # plane offsets would leave 32 bits
        assert call(**kw) == sfhip.SF_EINVAL, kw


def test_stream_window_refusals(L):
    import sfhip

    def call(ring=FAKE, s=S, head=0, fidx=FAKE, n_fast=4, sidx=FAKE, n_slow=2, fast=FAKE, slow=FAKE, hp=NEW_H + 2 * PH,
             wp=WP):
        return L.sf_stream_window(ring, s, head, fidx, n_fast, sidx, n_slow, fast, slow, hp, wp, None)

    for kw in (dict(ring=None), dict(fidx=None), dict(fast=None), dict(sidx=None),  # null pointers
               dict(slow=None),                                                    # n_slow > 0 with a null slow
               dict(n_slow=0),                                                     # ... and slow without n_slow
               dict(head=S), dict(head=-1), dict(s=0),
               dict(n_fast=0), dict(n_fast=-1), dict(n_fast=65536), dict(n_slow=-1), dict(n_slow=5),
               dict(hp=0), dict(wp=0), dict(hp=1 << 20, wp=1 << 12),
               dict(fast=ctypes.c_void_p(4104)), dict(slow=ctypes.c_void_p(4104)), dict(ring=ctypes.c_void_p(4104))):
        assert call(**kw) == sfhip.SF_EINVAL, kw


def test_label_select_refusals(L):
    import sfhip
    ip = ctypes.cast(FAKE, ctypes.POINTER(ctypes.c_int))

    def call(preds=FAKE, r=1, c=5, thr=0.1, out=ip):
        return L.sf_label_select(preds, r, c, thr, out, None)

    for kw in (dict(preds=None), dict(out=None), dict(c=0), dict(c=-1), dict(r=0), dict(r=-1),
               dict(thr=float("nan")), dict(preds=ctypes.c_void_p(4098)),
               dict(out=ctypes.cast(ctypes.c_void_p(4098), ctypes.POINTER(ctypes.c_int)))):
        assert call(**kw) == sfhip.SF_EINVAL, kw
