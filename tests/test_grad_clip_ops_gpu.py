"""Gradient clipping on the GPU (csrc/grad_clip.hip through slowfast/models/step_tail.py::HipGradClip) against numpy
float64 on the host, computed from the very float32 gradients the kernels read.

One parameter set: numels 1, 3, 4, 5, 4095, 4096, 4097, 8193 (the chunk is 4096 elements: chunk edges, tails of 1-3
elements, up to three chunks per tensor), every gradient a view of ONE allocation with four canary floats in front of and
behind it; the 4097-element gradient starts one float past a 16-byte boundary (both of its chunks take the 4-byte path),
the others on one; one more parameter has `.grad = None`.

Bounds.  Norm 2: every element passes through at most 16 sequential + 6 butterfly + 3 LDS additions in its chunk and
1 + 6 + 3 in the finish (<= 256 chunks), all of non-negative fp64 terms, plus one rounding of the square and one sqrt:
under 64 * 2^-53 ~ 7e-15 relative; asserted at 1e-13.  Scaled gradients: one fp32 rounding of the coefficient and one of
the product, 2^-24 each, so 2^-23; asserted at 2^-22 of |g c|.
Measured on an MI355X (profiles/grad_clip.txt): norm error 0; scaled gradients 6.8e-08 (norm 2), 6.0e-08 (norm inf)."""
import math

import numpy as np
import pytest
import torch

from _host_reads import count_host_reads

pytestmark = pytest.mark.gpu
NUMELS = [1, 3, 4, 5, 4095, 4096, 4097, 8193]
MISALIGNED = 6         # index of the gradient that starts one float past a 16-byte boundary
CANARY = 4             # floats in front of and behind every gradient
CANARY_VALUE = 12345.678


class _Set(object):
    """The parameter set: `buf` holds canaries and gradients, `buf0` the values it started from."""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        spans, n = [], CANARY
        for i, k in enumerate(NUMELS):
            n = (n + 3) // 4 * 4 + (1 if i == MISALIGNED else 0)
            spans.append((n, k))
            n += k + CANARY
        host = torch.full((n + CANARY,), CANARY_VALUE)
        self.mask = torch.ones(host.numel(), dtype=torch.bool)   # True: a canary
        for s, k in spans:
            # magnitudes from 1e-3 to 10: the sum is not dominated by one tensor, nothing is near the subnormals
            host[s:s + k] = torch.randn(k, generator=g) * 10.0 ** float(torch.empty(1).uniform_(-3, 1, generator=g))
            self.mask[s:s + k] = False
        self.spans = spans
        self.buf0 = host.clone()
        self.buf = host.cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.params = []
        for s, k in spans:
            p = torch.nn.Parameter(torch.randn(k, generator=g).cuda())
            p.grad = self.buf[s:s + k]
            self.params.append(p)
        for i, p in enumerate(self.params):
            assert (p.grad.data_ptr() % 16 == 0) == (i != MISALIGNED) and p.grad.data_ptr() % 4 == 0
        self.absent = torch.nn.Parameter(torch.randn(37, generator=g).cuda())   # .grad stays None
        self.absent0 = self.absent.detach().clone()
        self.all = self.params[:4] + [self.absent] + self.params[4:]

    def refill(self, host=None):
        self.buf.copy_(self.buf0 if host is None else host)

    def grads64(self, host=None):
        h = (self.buf0 if host is None else host).numpy()
        return [h[s:s + k].astype(np.float64) for s, k in self.spans]

    def norm2(self, host=None):
        return math.sqrt(math.fsum(float(v) * float(v) for g in self.grads64(host) for v in g))

    def check_untouched_surroundings(self):
        got = self.buf.cpu()
        assert torch.equal(got[self.mask].view(torch.int32), self.buf0[self.mask].view(torch.int32)), "canaries"
        assert torch.equal(self.absent.detach(), self.absent0) and self.absent.grad is None


@pytest.fixture(scope="module")
def pset():
    return _Set()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _clipper(ps, **kw):
    from slowfast.models.step_tail import HipGradClip
    return HipGradClip(ps.all, **kw)


def test_norm2_is_the_fp64_norm(pset):
    pset.refill()
    clip = _clipper(pset, max_norm=1e30)
    out = clip.clip()
    torch.cuda.synchronize()
    ref = pset.norm2()
    got = float(clip.total_norm64.cpu()[0])
    rel = abs(got - ref) / ref
    print("norm2: got %.17g ref %.17g rel err %.3e" % (got, ref, rel))
    assert rel <= 1e-13
    assert out.data_ptr() == clip.total_norm.data_ptr()
    assert _bits(clip.total_norm).item() == torch.tensor(got, dtype=torch.float64).float().view(torch.int32).item()
    assert float(clip.nonfinite.cpu()[0]) == 0.0 and float(clip.guard.cpu()[0]) == 0.0
    pset.check_untouched_surroundings()


def test_norm_inf_is_the_largest_magnitude(pset):
    pset.refill()
    clip = _clipper(pset, max_norm=1e30, norm_type=float("inf"))
    clip.clip()
    torch.cuda.synchronize()
    ref = max(float(np.abs(g).max()) for g in pset.grads64())
    assert float(clip.total_norm64.cpu()[0]) == ref
    assert float(clip.total_norm.cpu()[0]) == ref           # a float32's magnitude: exact in both
    assert float(clip.coef.cpu()[0]) == 1.0


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
def test_scaled_gradients_and_their_surroundings(pset, norm_type):
    pset.refill()
    g64 = pset.grads64()
    norm = pset.norm2() if norm_type == 2.0 else max(float(np.abs(g).max()) for g in g64)
    max_norm = float(np.float32(0.5 * norm))                 # what the kernel reads: a float32
    clip = _clipper(pset, max_norm=max_norm, norm_type=norm_type)
    clip.clip()
    torch.cuda.synchronize()
    c = min(1.0, max_norm / (norm + 1e-6))
    assert 0.4 < c < 0.6
    first = pset.buf.clone()
    worst = 0.0
    for p, g in zip(pset.params, g64):
        want = g * c
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float((err / np.abs(want)).max()))
        assert (err <= 2.0 ** -22 * np.abs(want)).all()
    print("scale (norm %s): coefficient %.17g, worst relative error %.3e (bound %.3e)" % (norm_type, c, worst, 2.0 ** -22))
    assert abs(float(clip.coef.cpu()[0]) - c) <= 2.0 ** -24 * c
    pset.check_untouched_surroundings()
    # the same gradients again: the same bits
    pset.refill()
    clip.clip()
    torch.cuda.synchronize()
    assert torch.equal(_bits(pset.buf), _bits(first))


def test_no_clipping_touches_nothing(pset):
    pset.refill()
    clip = _clipper(pset, max_norm=float(np.float32(1.5 * pset.norm2())))
    clip.clip()
    torch.cuda.synchronize()
    assert _bits(clip.coef).item() == torch.tensor(1.0).view(torch.int32).item()
    assert torch.equal(_bits(pset.buf), pset.buf0.view(torch.int32))


@pytest.mark.parametrize("norm_type", [2.0, float("inf")])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_non_finite_gradient_raises_the_guard_and_moves_nothing(pset, poison, norm_type):
    from slowfast.models.step_tail import HipSGD
    pset.refill()
    opt = HipSGD(pset.all, lr=0.1, momentum=0.9, weight_decay=1e-3)
    clip = _clipper(pset, max_norm=float(np.float32(0.5 * pset.norm2())), norm_type=norm_type)
    clip.clip()
    opt.step(guard=clip.guard)                               # a good step first: the momentum buffers exist
    torch.cuda.synchronize()
    assert float(clip.guard.cpu()[0]) == 0.0
    bufs = [opt.state[p]["momentum_buffer"] for p in pset.params]
    p0 = [_bits(p) for p in pset.params]
    m0 = [_bits(b) for b in bufs]
    host = pset.buf0.clone()
    s, k = pset.spans[5]
    host[s + 2077] = poison                                  # inside the 4096-element gradient
    pset.refill(host)
    clip.clip()
    opt.step(guard=clip.guard)
    torch.cuda.synchronize()
    assert float(clip.nonfinite.cpu()[0]) != 0.0 and float(clip.guard.cpu()[0]) != 0.0
    assert not math.isfinite(float(clip.total_norm.cpu()[0]))
    assert torch.equal(_bits(pset.buf), host.view(torch.int32)), "the gradients are left exactly as they are"
    assert all(torch.equal(_bits(p), a) for p, a in zip(pset.params, p0))
    assert all(torch.equal(_bits(b), a) for b, a in zip(bufs, m0))
    # finite again: the guard falls and the step goes through
    pset.refill()
    clip.clip()
    opt.step(guard=clip.guard)
    torch.cuda.synchronize()
    assert float(clip.guard.cpu()[0]) == 0.0
    assert not any(torch.equal(_bits(p), a) for p, a in zip(pset.params, p0))


def test_a_raised_loss_guard_stays_raised_and_nothing_is_scaled(pset):
    pset.refill()
    clip = _clipper(pset, max_norm=float(np.float32(0.5 * pset.norm2())))
    for raised in (1.0, float("nan")):
        guard = torch.tensor([raised]).cuda()
        clip.clip(guard=guard)
        torch.cuda.synchronize()
        assert float(clip.guard.cpu()[0]) == 1.0 and float(clip.nonfinite.cpu()[0]) == 0.0
        assert 0.4 < float(clip.coef.cpu()[0]) < 0.6         # it would have scaled
        assert torch.equal(_bits(pset.buf), pset.buf0.view(torch.int32))
    clip.clip(guard=torch.zeros(1).cuda())
    torch.cuda.synchronize()
    assert float(clip.guard.cpu()[0]) == 0.0
    assert not torch.equal(_bits(pset.buf), pset.buf0.view(torch.int32))


def test_clip_value_is_torch_clamp_bit_for_bit(pset):
    host = pset.buf0.clone()
    # the median magnitude (a float32): about half of the elements move
    v = float(torch.cat([pset.buf0[s:s + k] for s, k in pset.spans]).abs().median())
    specials = [float("nan"), float("inf"), -float("inf"), -0.0, 0.0, v, -v]
    for i, (s, k) in enumerate(pset.spans):
        for j, special in enumerate(specials):
            if j < k:
                host[s + (j * 611) % k] = special            # spread over chunks, vector bodies and tails
    s, k = pset.spans[MISALIGNED]
    host[s + k - 1] = float("nan")                           # the last element of the 4-byte path
    pset.refill(host)
    clip = _clipper(pset, clip_value=v)
    assert clip.clip() is None
    torch.cuda.synchronize()
    want = host.clone()
    moved = 0
    for s, k in pset.spans:
        want[s:s + k] = torch.clamp(host[s:s + k], -v, v)
        moved += int((want[s:s + k] != host[s:s + k]).sum())
    assert moved > 1000
    assert torch.equal(_bits(pset.buf), want.view(torch.int32))  # the canaries (12345.678 > v) are not clamped
    pset.check_untouched_surroundings()
    # both at once: the clamp first, then the norm of the clamped gradients
    pset.refill()
    both = _clipper(pset, clip_value=v, max_norm=1e30)
    both.clip()
    torch.cuda.synchronize()
    clamped = pset.buf0.clone()
    for s, k in pset.spans:
        clamped[s:s + k] = torch.clamp(pset.buf0[s:s + k], -v, v)
    ref = pset.norm2(clamped)
    assert abs(float(both.total_norm64.cpu()[0]) - ref) <= 1e-13 * ref


def test_ring_gets_the_norm_in_column_7_of_the_steps_row(pset):
    from slowfast.models.step_tail import HipCrossEntropy, StatsRing
    pset.refill()
    ring = StatsRing(3)
    clip = _clipper(pset, max_norm=1e30, ring=ring)
    ring.rows.fill_(7.75)
    clip.clip()                                              # a fresh ring (counter 0): nothing is written
    torch.cuda.synchronize()
    assert int(ring.counter.cpu()[0]) == 0 and bool((ring.rows == 7.75).all())
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(4, 9, generator=g).cuda().requires_grad_(True)
    labels = torch.randint(0, 9, (4,), generator=g).cuda()
    loss_fun = HipCrossEntropy(1, ring)
    for step in range(4):                                    # the fourth wraps around to row 0
        loss_fun(logits, labels)
        torch.cuda.synchronize()
        before = ring.rows.clone()
        row = step % 3
        assert float(before[row, 7]) == 0.0 and int(ring.counter.cpu()[0]) == step + 1
        clip.clip(guard=loss_fun.guard)
        torch.cuda.synchronize()
        want = before.clone()
        want[row, 7] = clip.total_norm[0]
        assert torch.equal(_bits(ring.rows), _bits(want))
        assert float(ring.rows[row, 7]) == float(np.float32(float(clip.total_norm64.cpu()[0]))) > 0.0
        assert int(ring.counter.cpu()[0]) == step + 1


def test_no_host_read_inside_clip(pset):
    pset.refill()
    clip = _clipper(pset, max_norm=float(np.float32(0.5 * pset.norm2())), clip_value=5.0)
    clip.clip()
    torch.cuda.synchronize()
    import sfhip
    calls = sfhip.CALLS
    with count_host_reads() as seen:
        clip.clip()
        clip.clip(guard=clip.nonfinite)
    torch.cuda.synchronize()
    assert seen == []
    assert sfhip.CALLS == calls + 6                          # clamp, norm, scale — nothing rebuilt, nothing uploaded


def test_captured_clip_and_step_replays_the_eager_bits(pset):
    from slowfast.models import engine
    from slowfast.models.step_tail import HipSGD
    pset.refill()
    second = _Set(seed=1).buf0                               # new gradient values for the same buffers
    scale = float(np.float32(0.5 * pset.norm2(second)))
    side = torch.cuda.Stream()

    def make():
        for p, (s, k) in zip(pset.params, pset.spans):
            with torch.no_grad():
                p.copy_(pset.buf0[s:s + k].flip(0))
        opt = HipSGD(pset.all, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)
        clip = _clipper(pset, max_norm=scale)

        def step():
            clip.clip()
            opt.step(guard=clip.guard)
        with torch.cuda.stream(side):
            for _ in range(2):                               # eager warm-up: tables, momentum buffers, uploads
                pset.refill()
                step()
        torch.cuda.synchronize()
        return opt, clip, step

    opt, clip, step = make()
    with torch.cuda.stream(side):
        pset.refill(second)
        step()
    torch.cuda.synchronize()
    eager = ([_bits(p) for p in pset.params], [_bits(opt.state[p]["momentum_buffer"]) for p in pset.params],
             _bits(pset.buf), _bits(clip.total_norm))
    assert float(clip.coef.cpu()[0]) < 0.6

    opt, clip, step = make()
    graph = torch.cuda.CUDAGraph()
    before = [_bits(p) for p in pset.params]
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), b) for p, b in zip(pset.params, before)), "a capture runs nothing"
    with torch.cuda.stream(side):
        pset.refill(second)
        engine.replay(graph)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p), e) for p, e in zip(pset.params, eager[0]))
    assert all(torch.equal(_bits(opt.state[p]["momentum_buffer"]), e) for p, e in zip(pset.params, eager[1]))
    assert torch.equal(_bits(pset.buf), eager[2]) and torch.equal(_bits(clip.total_norm), eager[3])

    # a gradient at a new address needs a new table: refused under capture
    moved = pset.params[2]
    moved.grad = moved.grad.clone()
    try:
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="warm up eagerly"):
            with torch.cuda.graph(graph, stream=side):
                clip.clip()
        torch.cuda.synchronize()
    finally:
        s, k = pset.spans[2]
        moved.grad = pset.buf[s:s + k]
