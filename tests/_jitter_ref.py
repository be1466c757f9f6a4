"""Jester's colour jitter (the reference's transform.RandomColorJitter, transform.py:692-717: PIL's
ImageEnhance.Brightness, then Contrast, then Color) restated in numpy, uint8 frame in and uint8 frame out — the contract
include/sfhip.h states for sf_clip_batch_jitter, in integers and float32, so every comparison against it is exact.

    blend(f, x0, x1) = fl32(x0 + fl32(f * (x1 - x0))), truncated toward zero for 0 <= f <= 1, otherwise clipped to
                       [0, 255] and truncated; f is the factor as a C float
    grey(c)          = (19595 c0 + 38470 c1 + 7471 c2 + 32768) >> 16
    frame mean m     = (2 S + n) / (2 n), S the sum of grey(.) over the whole brightness-jittered frame of n pixels
"""
import numpy as np


def blend(f, x0, x1):
    """PIL's Image.blend(x0, x1, f) on uint8 arrays (or scalars) -> uint8 array."""
    f = np.float32(f)
    x0 = np.asarray(x0).astype(np.int32)
    x1 = np.asarray(x1).astype(np.int32)
    prod = (f * (x1 - x0).astype(np.float32)).astype(np.float32)      # one rounded product
    t = (x0.astype(np.float32) + prod).astype(np.float32)             # one rounded sum
    if 0.0 <= float(f) <= 1.0:
        return t.astype(np.int32).astype(np.uint8)                    # truncation toward zero
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def grey(frame):
    """convert("L") of an [..., 3] uint8 array -> uint8 [...]."""
    c = frame.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16).astype(np.uint8)


def brightness(frame, fb):
    return blend(fb, np.zeros_like(frame), frame) if fb > 0 else frame


def grey_mean(frame, fb):
    """The mean ImageEnhance.Contrast blends against, for an [H, W, 3] uint8 frame after the brightness stage `fb`:
    int(ImageStat.Stat(L).mean[0] + 0.5) in integers."""
    g = grey(brightness(frame, fb))
    S, n = int(g.astype(np.int64).sum()), g.size
    return (2 * S + n) // (2 * n)


def jitter_frame(frame, bright, contrast, color):
    """RandomColorJitter(bright, contrast, color)._jitter on one [H, W, 3] uint8 frame -> uint8 [H, W, 3]."""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    out = brightness(frame, bright)
    if contrast > 0:
        out = blend(contrast, np.full_like(out, grey_mean(frame, bright)), out)
    if color > 0:
        out = blend(color, np.repeat(grey(out)[..., None], 3, axis=2), out)
    return out


def jitter_clip(clip, bright, contrast, color):
    """Every frame of a [T, H, W, 3] uint8 clip with the same three factors (the mean is each frame's own)."""
    return np.stack([jitter_frame(f, bright, contrast, color) for f in clip])
