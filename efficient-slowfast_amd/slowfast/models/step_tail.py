"""The training iteration behind the backward pass (reference tools/train_net.py:67-157) on libsfhip kernels.

* `StatsRing` — device memory the loss kernel writes one row of statistics into per step (loss, top-1 / top-k error,
  non-finite flag, batch size, bad-label count, loss kind); `utils.meters.DeviceTrainMeter` drains it once per LOG_PERIOD.
* `HipCrossEntropy(topk, ring)` — `loss_fun(preds, labels)` of train_net.py:84-87, `misc.check_nan_losses` (:90) and
  `metrics.topks_correct` (:122-125) as ONE launch (`sf_ce_topk`) with no host read.
* `HipBCE(ring)` / `HipBCEWithLogits(ring)` — `nn.BCELoss(reduction="mean")` on probabilities (detection, losses.py
  "bce") and `nn.BCEWithLogitsLoss(reduction="mean")` on logits (multi-label classification, "bce_logit") with the
  NaN check as ONE launch (`sf_bce`); `get_hip_loss_func(cfg, ring)` picks by `MODEL.LOSS_FUNC`.
* Class weights — `HipCrossEntropy(..., weight=)`, `HipBCE(..., weight=)`, `HipBCEWithLogits(..., weight=, pos_weight=)`:
  `nn.CrossEntropyLoss(weight=)`, `nn.BCELoss(weight=)`, `nn.BCEWithLogitsLoss(weight=, pos_weight=)` as the same one
  launch (`sf_ce_topk_w`, `sf_bce_w`), the weights read from device memory at every step
  (`utils.meters.DevicePerClassMeter.class_weights(out=)` refreshes them in place, also under a captured step).
* Soft targets — `HipCrossEntropy(..., label_smoothing=)` and `loss_fun(preds, labels, mix=rows)`: label smoothing,
  mixup and CutMix (upstream's MIXUP.* and datasets/mixup.py) as the same one launch (`sf_ce_mix`) from the mix rows the
  input step already used (`datasets.utils.gpu_train_batch_mix`); `construct_hip_mixup(cfg)` draws the batch's mix.
* `topk_errors(preds, labels, k_hi, ring)` — the evaluation batch's row (train_net.py:227-232): `sf_topk_errors`, the same
  ring, no loss (`utils.meters.DeviceValMeter` drains it).
* `HipSGD` — `torch.optim.SGD` whose `step()` is ONE launch over every parameter of every group (`sf_sgd_step`), with the
  hyper-parameters in device memory: `optim.set_lr` (:68-69) stays a host assignment, `step()` / `upload_hyper()` turn a
  change into one small copy, and a captured step follows the schedule.
* `HipAdam` — `torch.optim.Adam` the same way (`sf_adam_step`: the step counts live in device memory and advance in a
  launch of their own in front of the update, so a replayed step keeps counting).
* `HipAdamW` — `torch.optim.AdamW`, HipAdam's kernel body with the decay decoupled (`sf_adamw_step`).
* `HipLARS` — HipSGD behind a layer-wise trust ratio (LARS / LARC): both norms of every tensor in two launches
  (`sf_lars_ratios`), then the SGD launch reading {r, wd_t} per tensor (`sf_lars_sgd_step`).
* `construct_hip_solver(model, cfg)` — models/optimizer.py:26-69: `construct_hip_optimizer` for `sgd`
  (`construct_hip_lars` with upstream's SOLVER.LARS_ON), `construct_hip_adam` for `adam`, `construct_hip_adamw` for
  upstream's `adamw`.
* `HipGradClip` — `torch.nn.utils.clip_grad_norm_` / `clip_grad_value_` between the backward pass and `step()`: a
  fixed-order fp64 global norm (`sf_grad_norm`), a scale launch that touches nothing when nothing needs clipping
  (`sf_grad_scale`), the value clamp (`sf_grad_clamp`); a non-finite gradient raises `.guard`, which `step(guard=)` takes.
  `construct_hip_grad_clip(model, cfg)` reads upstream's SOLVER.CLIP_GRAD_L2NORM / SOLVER.CLIP_GRAD_VAL.
There is no fallback: tensors that are not fp32 on the current GPU are refused."""
import ctypes

import torch

import sfhip

RING_ROW = 8
TAB_ROW, HYP_ROW = 6, 5
ADAM_TAB_ROW, ADAM_HYP_ROW = 7, 5
LARS_TAB_ROW, LARS_HYP_ROW = 6, 3
STAGE_SLOTS = 16
ROW_LOSS, ROW_TOP1, ROW_TOPK, ROW_FLAG, ROW_N, ROW_BAD, ROW_KIND = 0, 1, 2, 3, 4, 5, 6
KIND_CE, KIND_BCE, KIND_EVAL = 0, 1, 2  # ROW_KIND: which kernel wrote the row (2: sf_topk_errors, no loss)


class StatsRing(object):
    """`rows` float32 [cap, 8] and `counter` int32 [1] on `device` (a CPU ring serves the meter's tests).  Row
    `counter % cap` is the next one written; `counter` counts the steps since the ring was made."""

    def __init__(self, cap, device="cuda"):
        if int(cap) <= 0:
            raise ValueError("StatsRing: capacity must be positive, got %r" % (cap,))
        self.cap = int(cap)
        self.rows = torch.zeros((self.cap, RING_ROW), dtype=torch.float32, device=device)
        self.counter = torch.zeros((1,), dtype=torch.int32, device=device)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rows_view(t, N, K):
    """A [N, K] tensor the kernels can read in place (unit column stride, row stride >= K) and that row stride."""
    if N > 0 and K > 0 and (t.stride(1) != 1 or (N > 1 and t.stride(0) < K)):
        t = t.contiguous()
    return t, (t.stride(0) if N > 1 else K)


def _ce_args(who, preds, labels, host_args=None):
    """The checks of the [N, K] predictions + [N] labels family, in one order: the shapes, then `host_args(N, K)` (the
    caller's arguments that can be refused before anything needs the GPU), then the GPU, then the labels.  Returns the
    row view of preds, its leading dimension, the contiguous labels, N and K."""
    if preds.dim() != 2 or labels.dim() != 1 or labels.shape[0] != preds.shape[0]:
        raise ValueError("%s: preds [N, K] and labels [N], got %s and %s" % (who, tuple(preds.shape),
                                                                             tuple(labels.shape)))
    N, K = preds.shape
    if host_args is not None:
        host_args(N, K)
    sfhip._require_gpu(preds, who)
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise ValueError("%s: labels must be int64 on the GPU, got %s on %s" % (who, labels.dtype, labels.device))
    preds, ld = _rows_view(preds, N, K)
    return preds, int(ld), labels.contiguous(), N, K


def _bce_args(who, preds, targets, host_args=None):
    """The checks of the [N, K] predictions + [N, K] targets family, ordered as `_ce_args`; targets of any real dtype
    are converted to float32.  Returns both row views with their leading dimensions, N and K."""
    if preds.dim() != 2 or tuple(targets.shape) != tuple(preds.shape):
        raise ValueError("%s: preds [N, K] and targets [N, K], got %s and %s" % (who, tuple(preds.shape),
                                                                                 tuple(targets.shape)))
    N, K = preds.shape
    if host_args is not None:
        host_args(N, K)
    sfhip._require_gpu(preds, who)
    if not targets.is_cuda:
        raise sfhip.SfhipError("%s: targets are on %s — the loss kernel runs on the GPU only" % (who, targets.device))
    if targets.dtype != torch.float32:
        targets = targets.float()
    sfhip._require_gpu(targets, who)
    preds, ldx = _rows_view(preds, N, K)
    targets, ldy = _rows_view(targets, N, K)
    return preds, int(ldx), targets, int(ldy), N, K


def _grad_out(N, K, given, out):
    """The gradient tensor of a loss launch: `given`, or a new fp32 [N, K] beside `out` (fp32 [2]: loss, flag)."""
    if given is None:
        given = torch.empty((N, K), dtype=torch.float32, device=out.device)
    assert given.is_contiguous() and tuple(given.shape) == (N, K) and out.numel() >= 2
    return given


def _ring_args(ring):
    """(rows pointer, counter pointer, capacity) of a StatsRing as the kernels take them; no ring: (None, None, 0)."""
    if ring is None:
        return None, None, 0
    return _vp(ring.rows), ctypes.cast(ctypes.c_void_p(ring.counter.data_ptr()), sfhip._pi), ring.cap


def ce_topk(preds, labels, k_hi, ring, out, dlogits=None):
    """One `sf_ce_topk` launch.  preds fp32 [N, K] (unit column stride, row stride >= K), labels int64 [N], out fp32 [2]
    (loss, non-finite flag).  Returns dlogits [N, K]."""
    preds, ld, labels, N, K = _ce_args("ce_topk", preds, labels)
    dlogits = _grad_out(N, K, dlogits, out)
    sfhip._call("sf_ce_topk", _vp(preds), ld, _vp(labels), N, K, int(k_hi), _vp(dlogits), *_ring_args(ring), _vp(out),
                tag="ce_topk")
    return dlogits


def bce(preds, targets, from_logits, ring, out, dgrad=None):
    """One `sf_bce` launch.  preds fp32 [N, K] (probabilities, or logits with from_logits), targets [N, K] of any
    real dtype (the reference's label tensors are float64 or integer: converted to float32), both as row views (unit
    column stride, row stride >= K); out fp32 [2] (loss, non-finite flag).  Returns d loss / d preds [N, K]."""
    preds, ldx, targets, ldy, N, K = _bce_args("bce", preds, targets)
    dgrad = _grad_out(N, K, dgrad, out)
    sfhip._call("sf_bce", _vp(preds), ldx, _vp(targets), ldy, N, K, 1 if from_logits else 0, _vp(dgrad),
                *_ring_args(ring), _vp(out), tag="bce")
    return dgrad


def _weight_vector(t, K, device, who, name):
    """fp32 [K], contiguous, on `device` — what the weighted kernels read; anything else is a ValueError."""
    if not torch.is_tensor(t):
        raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != K or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous float32 tensor of shape (%d,), got %s %s" % (
            who, name, K, t.dtype, tuple(t.shape)))
    if t.device != device:
        raise ValueError("%s: %s is on %s, the predictions on %s" % (who, name, t.device, device))
    return t


def ce_topk_w(preds, labels, weight, k_hi, ring, out, dlogits=None):
    """One `sf_ce_topk_w` launch: `ce_topk` with class weights, F.cross_entropy(weight=) — the divisor is the sum of
    the rows' weights.  weight fp32 [K], contiguous, on the predictions' GPU."""
    preds, ld, labels, N, K = _ce_args(
        "ce_topk_w", preds, labels, lambda N, K: _weight_vector(weight, K, preds.device, "ce_topk_w", "weight"))
    dlogits = _grad_out(N, K, dlogits, out)
    sfhip._call("sf_ce_topk_w", _vp(preds), ld, _vp(labels), _vp(weight), N, K, int(k_hi), _vp(dlogits),
                *_ring_args(ring), _vp(out), tag="ce_topk_w")
    return dlogits


def _smoothing(v, who):
    """label smoothing as the kernel takes it: a number in [0, 1)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s: label smoothing must be a number in [0, 1), got %r" % (who, v))
    if not 0.0 <= f < 1.0:  # (a NaN fails both)
        raise ValueError("%s: label smoothing must lie in [0, 1), got %r" % (who, v))
    return f


def _mix_pair(mix_host, mix, N, who):
    """The mix rows of `N` predictions as the loss entry takes them: int64 [N, 7], contiguous — `mix` on the GPU, `mix_host`
    the host copy it was uploaded from.  Both None: no mixing."""
    if mix is None and mix_host is None:
        return None, None
    if mix is None or mix_host is None:
        raise ValueError("%s: mix rows come as a pair — the device rows and the host copy they were uploaded from" % who)
    for name, t in (("mix_host", mix_host), ("mix", mix)):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (N, sfhip.SF_MIX_ROW) or \
                not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous int64 tensor of shape (%d, %d), got %s %s" % (
                who, name, N, sfhip.SF_MIX_ROW, getattr(t, "dtype", type(t).__name__),
                tuple(getattr(t, "shape", ()))))
    if mix_host.device.type != "cpu":
        raise ValueError("%s: mix_host is the HOST copy of the rows, got a tensor on %s" % (who, mix_host.device))
    return mix_host, mix


def ce_mix(preds, labels, k_hi, ring, out, mix_host=None, mix=None, smoothing=0.0, dlogits=None):
    """One `sf_ce_mix` launch: `ce_topk` on the soft targets of label smoothing (`smoothing` in [0, 1)), mixup and
    CutMix — F.cross_entropy(preds, t) with t = (1 - eps) (lam onehot(a) + (1 - lam) onehot(b)) + eps / K, a the row's
    label, b its partner's.  mix: the device rows int64 [N, 7] `gpu_train_batch_mix` returns (partner, mode, lam as
    float32 bits, box), mix_host their host copy; both None: no mixing."""
    def host_args(N, K):
        _smoothing(smoothing, "ce_mix")
        _mix_pair(mix_host, mix, N, "ce_mix")

    preds, ld, labels, N, K = _ce_args("ce_mix", preds, labels, host_args)
    if mix is not None and not mix.is_cuda:
        raise sfhip.SfhipError("ce_mix: the mix rows are on %s — the loss kernel runs on the GPU only" % mix.device)
    dlogits = _grad_out(N, K, dlogits, out)
    sfhip._call("sf_ce_mix", _vp(preds), ld, _vp(labels), _vp(mix_host), _vp(mix), N, K, int(k_hi), float(smoothing),
                _vp(dlogits), *_ring_args(ring), _vp(out), tag="ce_mix")
    return dlogits


def bce_w(preds, targets, from_logits, ring, out, weight=None, pos_weight=None, dgrad=None):
    """One `sf_bce_w` launch: `bce` with nn.BCELoss(weight=) / nn.BCEWithLogitsLoss(weight=, pos_weight=).  weight and
    pos_weight fp32 [K], contiguous, on the predictions' GPU, or None (all ones); pos_weight needs from_logits."""
    def host_args(N, K):
        if pos_weight is not None and not from_logits:
            raise ValueError("bce_w: pos_weight belongs to the loss on logits (nn.BCEWithLogitsLoss); nn.BCELoss has "
                             "none")
        for name, w in (("weight", weight), ("pos_weight", pos_weight)):
            if w is not None:
                _weight_vector(w, K, preds.device, "bce_w", name)

    preds, ldx, targets, ldy, N, K = _bce_args("bce_w", preds, targets, host_args)
    dgrad = _grad_out(N, K, dgrad, out)
    sfhip._call("sf_bce_w", _vp(preds), ldx, _vp(targets), ldy, _vp(weight), _vp(pos_weight), N, K,
                1 if from_logits else 0, _vp(dgrad), *_ring_args(ring), _vp(out), tag="bce_w")
    return dgrad


def topk_errors(preds, labels, k_hi, ring):
    """One `sf_topk_errors` launch: the top-1 / top-k_hi errors of an evaluation batch (train_net.py:227-232) as a ring
    row of kind KIND_EVAL.  preds fp32 [N, K] (unit column stride, row stride >= K), labels int64 [N]."""
    preds, ld, labels, N, K = _ce_args("topk_errors", preds, labels)
    sfhip._call("sf_topk_errors", _vp(preds), ld, _vp(labels), N, K, int(k_hi), *_ring_args(ring), tag="topk_errors")


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, labels, owner):
        d = owner._launch(preds.detach(), labels)
        owner.dlogits = d
        ctx.save_for_backward(d)
        return owner.out[0].clone() if owner.keep_loss else owner.out[0]

    @staticmethod
    def backward(ctx, grad_output):
        (d,) = ctx.saved_tensors
        return d * grad_output, None, None


class _HipLoss(object):
    """A loss whose value, gradient, ring row and flag come from one launch: `loss = loss_fun(preds, labels)`;
    `loss.backward()` as in the reference, or `.backward_direct(preds)` to hand the stored gradient to autograd without
    the multiply by grad_output (= 1).  `guard` is the step's non-finite flag at a fixed address:
    `optimizer.step(guard=loss_fun.guard)`.  The returned loss is a view of a buffer the next call overwrites
    (keep_loss=True returns a copy, one more launch)."""

    def __init__(self, ring, keep_loss=False):
        self.ring, self.keep_loss = ring, bool(keep_loss)
        self.out = torch.zeros((2,), dtype=torch.float32, device=ring.rows.device)
        self.dlogits = None  # d loss / d preds of the last call

    @property
    def guard(self):
        return self.out[1:2]

    def __call__(self, preds, labels):
        return _LossFunction.apply(preds, labels, self)

    def backward_direct(self, preds):
        if self.dlogits is None or tuple(self.dlogits.shape) != tuple(preds.shape):
            raise RuntimeError("%s.backward_direct: call the loss on these predictions first" % type(self).__name__)
        preds.backward(gradient=self.dlogits)


def _as_weight(w, device, who, name):
    """A weight argument of a loss object -> the tensor the kernel reads.  A tensor is kept as it is — a REFERENCE, so a
    captured step sees values refreshed in place; a host list / numpy array is checked once (one dimension, finite,
    non-negative) and uploaded.  The length is checked against K at the first call."""
    if w is None:
        return None
    if torch.is_tensor(w):
        if w.dtype != torch.float32 or w.dim() != 1 or not w.is_contiguous():
            raise ValueError("%s: %s must be a contiguous one-dimensional float32 tensor, got %s %s" % (
                who, name, w.dtype, tuple(w.shape)))
        if w.device != torch.device(device):
            raise ValueError("%s: %s is on %s, the ring on %s" % (who, name, w.device, device))
        return w
    import numpy as np
    try:
        host = np.asarray(w, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: %s must be a float32 tensor or a sequence of numbers, got %r" % (who, name, w))
    if host.ndim != 1 or host.size == 0:
        raise ValueError("%s: %s must have one dimension [K], got shape %s" % (who, name, host.shape))
    if not np.isfinite(host).all() or (host < 0).any():
        raise ValueError("%s: %s must be finite and non-negative, got %s" % (who, name, host.tolist()))
    return torch.tensor(host, dtype=torch.float32).to(device)


def _set_weight(cur, new, who, name):
    if cur is None:
        raise ValueError("%s.set_%s: the loss was made without %s" % (who, name, name))
    new = torch.as_tensor(new)
    if tuple(new.shape) != tuple(cur.shape):
        raise ValueError("%s.set_%s: shape %s, the loss holds %s" % (who, name, tuple(new.shape), tuple(cur.shape)))
    cur.copy_(new)


class HipCrossEntropy(_HipLoss):
    """`HipCrossEntropy(cfg.TRAIN.TOPK, ring)`: softmax cross-entropy with the meter's top-1 / top-k errors.

    `weight` (fp32 [K] on the ring's device, or a host list / numpy array uploaded once): nn.CrossEntropyLoss(weight=)
    as the same one launch (`sf_ce_topk_w`).  A tensor is kept by reference — `class_weights(out=weight)` once per epoch
    or `set_weight(t)` (a `copy_`) change what the next step, captured or not, reads.  With several GPUs every rank
    divides by the weight sum of ITS rows and DDP averages the gradients, exactly what nn.CrossEntropyLoss(weight=) does
    under DDP: that is not the weighted mean over the global batch.

    `label_smoothing` (a number in [0, 1)) and `loss_fun(preds, labels, mix=rows)`: soft targets — label smoothing,
    mixup and CutMix (upstream's MIXUP.LABEL_SMOOTH_VALUE and datasets/mixup.py) — as the same one launch (`sf_ce_mix`);
    the errors are counted against each row's dominant label.  `mix` is the [N, 7] int64 device tensor
    `datasets.utils.gpu_train_batch_mix` returns (its `mix_host` attribute is the host copy the entry checks), or a
    `(host rows, device rows)` pair.  The device rows are taken by REFERENCE: a captured step reads whatever they hold
    when it is replayed, so copy each batch's rows into one fixed tensor (`fixed.copy_(rows)`); a tensor without a
    host copy is checked by the kernel alone (a row that fails there is a bad row: no loss, no gradient, counted).
    Class weights together with soft targets are refused: torch itself divides the two differently (by N for
    probability targets, by the weight sum for index targets).  With `label_smoothing == 0` and no `mix` the object
    launches `sf_ce_topk` / `sf_ce_topk_w` exactly as before."""

    def __init__(self, topk, ring, keep_loss=False, weight=None, label_smoothing=0.0):
        if int(topk) < 1:
            raise ValueError("HipCrossEntropy: topk must be at least 1, got %r" % (topk,))
        eps = _smoothing(label_smoothing, "HipCrossEntropy")
        if weight is not None and eps != 0.0:
            raise ValueError("HipCrossEntropy: weight together with label_smoothing is not supported — torch divides by "
                             "N for probability targets and by the weight sum for index targets")
        super().__init__(ring, keep_loss)
        self.topk = int(topk)
        self.weight = _as_weight(weight, ring.rows.device, "HipCrossEntropy", "weight")
        self.label_smoothing = eps
        self._mix = None        # the mix rows of the call in flight: (host rows, device rows)
        self._identity = None   # host rows that mix nothing, for device rows that come without a host copy

    def set_weight(self, t):
        _set_weight(self.weight, t, "HipCrossEntropy", "weight")

    def _host_rows(self, mix):
        """(host rows, device rows) of a `mix` argument."""
        if isinstance(mix, (tuple, list)):
            if len(mix) != 2:
                raise ValueError("HipCrossEntropy: mix is the device rows or a (host rows, device rows) pair")
            return mix[0], mix[1]
        if not torch.is_tensor(mix):
            raise ValueError("HipCrossEntropy: mix must be an int64 tensor [N, %d] or a (host, device) pair, got %s" % (
                sfhip.SF_MIX_ROW, type(mix).__name__))
        host = getattr(mix, "mix_host", None)
        if host is None and mix.dim() == 2:  # a fixed tensor refilled by the caller: the kernel's own check stands alone
            n = mix.shape[0]
            if self._identity is None or self._identity.shape[0] != n:
                ident = torch.zeros((n, sfhip.SF_MIX_ROW), dtype=torch.int64)
                ident[:, 0] = torch.arange(n)
                ident[:, 2] = 0x3f800000  # lam = 1.0f
                self._identity = ident
            host = self._identity
        return host, mix

    def __call__(self, preds, labels, mix=None):
        if mix is not None and self.weight is not None:
            raise ValueError("HipCrossEntropy: weight together with mix rows is not supported — torch divides by N for "
                             "probability targets and by the weight sum for index targets")
        self._mix = None if mix is None else self._host_rows(mix)
        try:
            return _LossFunction.apply(preds, labels, self)
        finally:
            self._mix = None

    def _launch(self, preds, labels):
        if self.label_smoothing != 0.0 or self._mix is not None:
            host, dev = self._mix if self._mix is not None else (None, None)
            return ce_mix(preds, labels, self.topk, self.ring, self.out, mix_host=host, mix=dev,
                          smoothing=self.label_smoothing)
        if self.weight is None:
            return ce_topk(preds, labels, self.topk, self.ring, self.out)
        return ce_topk_w(preds, labels, self.weight, self.topk, self.ring, self.out)


class HipBCE(_HipLoss):
    """`nn.BCELoss(reduction="mean")` on probabilities [N, K] (the detection head's output).  A batch without boxes
    ([0, K]) raises ValueError: the reference computes NaN there and stops on check_nan_losses.  `weight` (fp32 [K], as
    HipCrossEntropy takes it): nn.BCELoss(weight=), the mean over N K of weight[j] * loss (`sf_bce_w`)."""
    from_logits = False

    def __init__(self, ring, keep_loss=False, weight=None, pos_weight=None):
        who = type(self).__name__
        if pos_weight is not None and not self.from_logits:
            raise ValueError("%s: pos_weight belongs to the loss on logits (HipBCEWithLogits); nn.BCELoss has none" % who)
        super().__init__(ring, keep_loss)
        self.weight = _as_weight(weight, ring.rows.device, who, "weight")
        self.pos_weight = _as_weight(pos_weight, ring.rows.device, who, "pos_weight")

    def set_weight(self, t):
        _set_weight(self.weight, t, type(self).__name__, "weight")

    def set_pos_weight(self, t):
        _set_weight(self.pos_weight, t, type(self).__name__, "pos_weight")

    def _launch(self, preds, labels):
        if preds.dim() == 2 and preds.shape[0] * preds.shape[1] == 0:
            raise ValueError("%s: empty batch %s (a detection batch without boxes?) — the mean over no elements is "
                             "NaN" % (type(self).__name__, tuple(preds.shape)))
        if self.weight is None and self.pos_weight is None:
            return bce(preds, labels, self.from_logits, self.ring, self.out)
        return bce_w(preds, labels, self.from_logits, self.ring, self.out, weight=self.weight,
                     pos_weight=self.pos_weight)


class HipBCEWithLogits(HipBCE):
    """`nn.BCEWithLogitsLoss(reduction="mean")` on raw logits [N, K] (multi-label classification in training mode);
    `weight` / `pos_weight` (fp32 [K]) as nn.BCEWithLogitsLoss takes them."""
    from_logits = True


def _mixup_keys(cfg):
    """Upstream SlowFast's MIXUP node read with `.get` (config/defaults.py mirrors the reference's key set, which has no
    such node: add one to a config that allows new keys) -> (enable, alpha, cutmix_alpha, prob, switch_prob,
    label smoothing), upstream's defaults where a key is missing.  The smoothing counts only with MIXUP.ENABLE, as
    upstream, where the MixUp object is what smooths the labels."""
    node = getattr(cfg, "MIXUP", None)
    if node is None or not node.get("ENABLE", False):
        return False, 0.0, 0.0, 0.0, 0.0, 0.0
    return (True, float(node.get("ALPHA", 0.8)), float(node.get("CUTMIX_ALPHA", 1.0)), float(node.get("PROB", 1.0)),
            float(node.get("SWITCH_PROB", 0.5)), float(node.get("LABEL_SMOOTH_VALUE", 0.1)))


class HipMixUp(object):
    """The batch's mix decision with upstream's MIXUP.* settings: `mix = mixup.sample(B, crop)` (a
    `datasets.utils.MixParams`, drawn from numpy's global RNG in upstream's order) goes to
    `datasets.utils.gpu_train_batch_mix`, whose rows go to the loss; `label_smoothing` is what `get_hip_loss_func`
    hands to HipCrossEntropy."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1):
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.label_smoothing = _smoothing(label_smoothing, "HipMixUp")
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0 or not 0.0 <= self.prob <= 1.0 or \
                not 0.0 <= self.switch_prob <= 1.0:
            raise ValueError("HipMixUp: alphas must not be negative and the probabilities lie in [0, 1]")

    def sample(self, B, crop):
        from slowfast.datasets.utils import sample_mix_params
        return sample_mix_params(B, crop, self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob)


def construct_hip_mixup(cfg):
    """Upstream SlowFast's MIXUP.ENABLE / ALPHA / CUTMIX_ALPHA / PROB / SWITCH_PROB / LABEL_SMOOTH_VALUE as a HipMixUp, or
    None when the config has no MIXUP node or MIXUP.ENABLE is false."""
    enable, alpha, cutmix_alpha, prob, switch_prob, eps = _mixup_keys(cfg)
    if not enable:
        return None
    return HipMixUp(alpha, cutmix_alpha, prob, switch_prob, eps)


def get_hip_loss_func(cfg, ring, class_weights=None, pos_weight=None):
    """models/losses.py:20-28 by `cfg.MODEL.LOSS_FUNC`, on the kernels above.  `class_weights` / `pos_weight` (a tensor
    or a host sequence, [K]) give the weighted objects; "cross_entropy_weighted" — the name the reference keeps
    commented out in losses.py — is cross-entropy that requires `class_weights`.  There is no config key for the
    weights: config/defaults.py mirrors the reference's key set.  With upstream's MIXUP.ENABLE the cross-entropy takes
    MIXUP.LABEL_SMOOTH_VALUE (`construct_hip_mixup` draws the batch's mix)."""
    name = cfg.MODEL.LOSS_FUNC
    for what, w in (("class_weights", class_weights), ("pos_weight", pos_weight)):
        if w is not None and len(w) != cfg.MODEL.NUM_CLASSES:
            raise ValueError("Loss {}: {} of length {} for MODEL.NUM_CLASSES = {}".format(
                name, what, len(w), cfg.MODEL.NUM_CLASSES))
    if name in ("cross_entropy", "cross_entropy_weighted"):
        if name == "cross_entropy_weighted" and class_weights is None:
            raise ValueError("Loss cross_entropy_weighted needs class_weights")
        if pos_weight is not None:
            raise ValueError("Loss {}: pos_weight belongs to bce_logit".format(name))
        return HipCrossEntropy(cfg.TRAIN.TOPK, ring, weight=class_weights, label_smoothing=_mixup_keys(cfg)[5])
    if name == "bce":
        return HipBCE(ring, weight=class_weights, pos_weight=pos_weight)
    if name == "bce_logit":
        return HipBCEWithLogits(ring, weight=class_weights, pos_weight=pos_weight)
    raise NotImplementedError("Loss {} is not supported".format(name))


# ---------------------------------------------------------------------------------------------- address tables
def _build_tables(entries, chunk, row, numel_col):
    table = torch.tensor([list(map(int, e)) for e in entries], dtype=torch.int64).reshape(-1, row)
    rows = []
    for i, e in enumerate(entries):
        rows += [(i, s) for s in range(0, int(e[numel_col]), chunk)]
    return table, torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def build_sgd_tables(entries, chunk):
    """entries: (parameter address, gradient address, momentum address, numel, group, first) per tensor ->
    (table int64 [n, 6], chunks int64 [n_chunks, 2]): a chunk is (tensor index, first element) and covers at most
    `chunk` elements of one tensor; the chunks tile the tensors in order."""
    return _build_tables(entries, chunk, TAB_ROW, 3)


def build_adam_tables(entries, chunk):
    """entries: (parameter, gradient, exp_avg, exp_avg_sq, step address, numel, group) per tensor -> (table int64
    [n, 7], chunks int64 [n_chunks, 2]), tiled as build_sgd_tables does."""
    return _build_tables(entries, chunk, ADAM_TAB_ROW, 5)


def _tables_args(tag, table_host, table, chunks_host, chunks):
    """The six table and count arguments of every table entry; the host tensors are what the device ones were uploaded
    from."""
    for h, d in ((table_host, table), (chunks_host, chunks)):
        assert h.dtype == d.dtype == torch.int64 and h.is_contiguous() and d.is_contiguous() and not h.is_cuda, tag
        assert h.shape == d.shape, tag
    return (_vp(table_host), _vp(table), table_host.shape[0], _vp(chunks_host), _vp(chunks), chunks_host.shape[0])


def _table_step(symbol, dtype, table_host, table, chunks_host, chunks, hyper_host, hyper, guard, zero_grad):
    tag = symbol[3:]
    args = _tables_args(tag, table_host, table, chunks_host, chunks)
    assert hyper_host.dtype == hyper.dtype == dtype and hyper_host.shape == hyper.shape and hyper.is_contiguous()
    tag = symbol[3:]
    if not (table.is_cuda and chunks.is_cuda and hyper.is_cuda):
        raise sfhip.SfhipError("%s: table, chunks and hyper live on the GPU — there is no CPU fallback" % tag)
    sfhip._call(symbol, *args, _vp(hyper_host), _vp(hyper), hyper_host.shape[0], _vp(guard), 1 if zero_grad else 0,
                tag=tag)


def sgd_step(table_host, table, chunks_host, chunks, hyper_host, hyper, guard=None, zero_grad=False):
    """One `sf_sgd_step` launch; the host tensors are what the device ones were uploaded from."""
    _table_step("sf_sgd_step", torch.float32, table_host, table, chunks_host, chunks, hyper_host, hyper, guard,
                zero_grad)


def adam_step(table_host, table, chunks_host, chunks, hyper_host, hyper, guard=None, zero_grad=False):
    """One `sf_adam_step` call (two launches); hyper is float64 [n_groups, 5]."""
    _table_step("sf_adam_step", torch.float64, table_host, table, chunks_host, chunks, hyper_host, hyper, guard,
                zero_grad)


def build_lars_tables(entries, chunk):
    """entries: (parameter address, gradient address, numel, group, ignored) per tensor -> (table int64 [n, 6] with the
    index of the tensor's first chunk in column 4, chunks int64 [n_chunks, 2]), tiled as build_sgd_tables does."""
    rows, first = [], 0
    for p, g, numel, group, ignored in entries:
        rows.append((int(p), int(g), int(numel), int(group), first, 1 if ignored else 0))
        first += (int(numel) + chunk - 1) // chunk
    return _build_tables(rows, chunk, LARS_TAB_ROW, 2)


def lars_ratios(table_host, table, chunks_host, chunks, hyper_host, hyper, partials, ratios, state, guard=None):
    """One `sf_lars_ratios` call (two launches): {r, wd_t} of every tensor of the table into ratios (fp32 [n, 2]) and
    the guard into state (fp32 [8]: [4] non-finite flag, [5] guard_out).  hyper fp32 [n_groups + 1, 3] = lr,
    weight_decay, apply per group, then trust_coefficient, eps, clip; partials fp64 [n_chunks, 2]; guard the loss's
    (or the clipper's) guard or None."""
    args = _tables_args("lars_ratios", table_host, table, chunks_host, chunks)
    assert hyper_host.dtype == hyper.dtype == torch.float32 and hyper_host.shape == hyper.shape
    assert hyper.is_contiguous() and hyper_host.is_contiguous() and hyper_host.shape[0] >= 2
    if not (table.is_cuda and chunks.is_cuda and hyper.is_cuda and partials.is_cuda and ratios.is_cuda and state.is_cuda):
        raise sfhip.SfhipError("lars_ratios: tables, hyper, partials, ratios and state live on the GPU — there is no CPU "
                               "fallback")
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= 2 * chunks_host.shape[0]
    assert ratios.dtype == torch.float32 and ratios.is_contiguous() and ratios.numel() >= 2 * table_host.shape[0]
    assert state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= CLIP_STATE
    sfhip._call("sf_lars_ratios", *args, _vp(hyper_host), _vp(hyper), hyper_host.shape[0] - 1, _vp(guard),
                _vp(partials), _vp(ratios), _vp(state), tag="lars_ratios")


def lars_sgd_step(table_host, table, chunks_host, chunks, hyper_host, hyper, ratios, guard=None, zero_grad=False):
    """One `sf_lars_sgd_step` launch: `sgd_step` with {r, wd_t} per tensor from `ratios` (fp32 [n, 2] on the GPU)."""
    args = _tables_args("lars_sgd_step", table_host, table, chunks_host, chunks)
    assert hyper_host.dtype == hyper.dtype == torch.float32 and hyper_host.shape == hyper.shape
    assert hyper.is_contiguous() and hyper_host.is_contiguous()
    if not (table.is_cuda and chunks.is_cuda and hyper.is_cuda and ratios.is_cuda):
        raise sfhip.SfhipError("lars_sgd_step: table, chunks, hyper and ratios live on the GPU — there is no CPU "
                               "fallback")
    assert ratios.dtype == torch.float32 and ratios.is_contiguous() and ratios.numel() >= 2 * table_host.shape[0]
    sfhip._call("sf_lars_sgd_step", *args, _vp(hyper_host), _vp(hyper), hyper_host.shape[0], _vp(ratios), _vp(guard),
                1 if zero_grad else 0, tag="lars_sgd_step")


def adamw_step(table_host, table, chunks_host, chunks, hyper_host, hyper, guard=None, zero_grad=False):
    """One `sf_adamw_step` call (two launches); tables and hyper as `adam_step` takes them."""
    _table_step("sf_adamw_step", torch.float64, table_host, table, chunks_host, chunks, hyper_host, hyper, guard,
                zero_grad)


class _HyperStage(object):
    """The pinned staging ring of the hyper-parameter uploads.  The copy reads the staging row when the stream gets
    there, not now: every upload takes the next of STAGE_SLOTS pinned rows and leaves an event behind it, and a row is
    written again only after its event has passed (the host would have to run STAGE_SLOTS learning rates ahead of the
    device to wait here)."""

    def __init__(self):
        self._stage = None

    def upload(self, rows, dev_tensor):
        """One `non_blocking` copy of the host tensor `rows` into `dev_tensor` on the current stream."""
        if self._stage is None or self._stage.shape[1:] != rows.shape:
            self._stage = torch.empty((STAGE_SLOTS,) + tuple(rows.shape), dtype=rows.dtype).pin_memory()
            self._stage_events, self._stage_next = [None] * STAGE_SLOTS, 0
        i = self._stage_next
        self._stage_next = (i + 1) % STAGE_SLOTS
        if self._stage_events[i] is not None:
            self._stage_events[i].synchronize()
        self._stage[i].copy_(rows)
        dev_tensor.copy_(self._stage[i], non_blocking=True)
        self._stage_events[i] = torch.cuda.Event()
        self._stage_events[i].record()


def carve_views(numels, device):
    """One zero-filled float32 allocation holding a flat view of each of `numels` elements, every view on 16 bytes ->
    (the allocation, the views).  Shared by the optimizers' state slots and the averaged weights (models/weight_avg.py)."""
    offs, n = [], 0
    for k in numels:
        offs.append(n)
        n += (k + 3) // 4 * 4
    block = torch.zeros((n,), dtype=torch.float32, device=device)
    return block, [block[o:o + k] for o, k in zip(offs, numels)]


class _TableOptimizer(object):
    """What HipSGD and HipAdam share, mixed in in front of torch's optimizer: the parameter checks, 16-byte aligned
    state slots carved from allocations the optimizer owns, the address table cached by a cheap signature, the pinned
    staging ring of the hyper-parameter uploads, and the step around the one native call.  A subclass supplies
    `_REFUSED` (group options the kernel does not do), `_TORCH`, `_HYP_DTYPE`, `_KEY_COLS`, `_hyper_values`,
    `_check_hyper`, `_sig_extra`, `_entries`, `_build`, `_launch` and `_after_fresh`."""

    def _init_tables(self):
        self._refuse_groups()
        self._slots = {}          # parameter -> its view(s) of a state allocation
        self._blocks = []         # the allocations (one, unless groups or state were added later)
        self._key = None
        self._table = self._chunks = self._table_dev = self._chunks_dev = None
        self._hyper = self._hyper_dev = self._hyper_vals = None
        self._stage = _HyperStage()
        self._sig = self._plist = None  # what the table was built from; the flat parameter list
        self._check_params()

    def _refuse_groups(self):
        for g in self.param_groups:
            if any(g.get(k) for k in self._REFUSED):
                raise ValueError("%s: %s are not supported — use %s" % (self._NAME, " / ".join(self._REFUSED),
                                                                        self._TORCH))

    def _check_params(self):
        for g in self.param_groups:
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise ValueError("%s: parameter of dtype %s — float32 only" % (self._NAME, p.dtype))
                if not p.is_contiguous():
                    raise ValueError("%s: parameters must be contiguous" % self._NAME)

    def _carve(self, numels, device):
        """`carve_views` from an allocation this optimizer keeps."""
        block, views = carve_views(numels, device)
        self._blocks.append(block)
        return views

    def _invalidate(self):
        self._key = self._sig = self._plist = None

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, "_slots"):
            self._refuse_groups()
            self._check_params()
            self._invalidate()

    # ---- hyper-parameters in device memory
    def upload_hyper(self):
        """Copy the groups' hyper-parameters to the device if they changed since the last upload: one small copy on the
        current stream from a pinned staging row, so the host does not wait for the work already queued there.  Call
        it before `engine.replay(graph)`: a replayed step reads the values from device memory.  Returns whether
        anything was copied."""
        vals = self._hyper_values()
        if vals == self._hyper_vals:
            return False
        self._check_hyper()
        rows = torch.tensor(vals, dtype=self._HYP_DTYPE).reshape(len(vals), -1)
        dev = self.param_groups[0]["params"][0].device
        if self._hyper_dev is None or self._hyper_dev.shape != rows.shape:
            self._hyper_dev = torch.empty(rows.shape, dtype=self._HYP_DTYPE, device=dev)
        self._stage.upload(rows, self._hyper_dev)
        self._hyper, self._hyper_vals = rows, vals
        return True

    def _check_hyper(self):
        pass

    # ---- the step
    def _checked_grad(self, p):
        """p.grad if the kernel can read it (None: the parameter is absent from this step, as in torch)."""
        if p.grad is None:
            return None
        if not p.is_cuda:
            raise ValueError("%s: parameter on %s — the update kernel runs on the GPU only" % (self._NAME, p.device))
        if p.grad.is_sparse:
            raise ValueError("%s: sparse gradients are not supported — use %s" % (self._NAME, self._TORCH))
        if p.grad.dtype != torch.float32 or not p.grad.is_cuda or not p.grad.is_contiguous():
            raise ValueError("%s: gradients must be contiguous float32 tensors on the GPU" % self._NAME)
        return p.grad

    def _signature(self):
        """What the address table depends on, cheaply: every parameter's and gradient's address, the subclass's extra
        (which groups have momentum) and how many parameters have state.  Equal to the signature the table was built
        from = the table still holds (a state tensor re-assigned by hand is only seen at the next rebuild;
        load_state_dict and add_param_group force one)."""
        plist = self._plist
        if plist is None:
            plist = self._plist = [p for g in self.param_groups for p in g["params"]]
        grads = [p.grad for p in plist]
        return ([p.data_ptr() for p in plist], [0 if g is None else g.data_ptr() for g in grads],
                self._sig_extra(), len(self.state))

    @torch.no_grad()
    def step(self, closure=None, guard=None, zero_grad=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sig = self._signature()
        if sig != self._sig:  # first call, or an address / a group changed: check everything and rebuild the table
            entries, fresh = self._entries()
            if not entries:
                return loss
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s.step under stream capture needs a new address table or a parameter's first "
                                   "step, which take host-to-device copies — warm up eagerly first (run the same step "
                                   "outside the capture until every parameter has had one)" % self._NAME)
            key = tuple(e[:self._KEY_COLS] for e in entries)
            self._table, chunks = self._build(entries, sfhip.lib().sf_sgd_chunk_elems())
            dev = self.param_groups[0]["params"][0].device
            self._table_dev = self._table.to(dev)
            if key != self._key:
                self._chunks, self._chunks_dev = chunks, chunks.to(dev)
            self._key = key
        else:
            fresh = ()
        if not torch.cuda.is_current_stream_capturing():
            self.upload_hyper()
        elif self._hyper_dev is None:
            raise RuntimeError("%s.step under stream capture: warm up eagerly first" % self._NAME)
        if guard is not None and (not guard.is_cuda or guard.dtype != torch.float32):
            raise ValueError("%s.step: guard is a float32 tensor on the GPU" % self._NAME)
        self._launch(self._table, self._table_dev, self._chunks, self._chunks_dev, self._hyper, self._hyper_dev, guard,
                     zero_grad)
        if fresh:
            self._after_fresh(fresh)
            sig = self._signature()  # the state grew
        self._sig = sig
        return loss


# ---------------------------------------------------------------------------------------------------------- SGD
class HipSGD(_TableOptimizer, torch.optim.SGD):
    """torch.optim.SGD (same constructor, param_groups and state_dict) with a one-launch `step()`.

    Momentum buffers are 16-byte aligned views of one allocation owned by the optimizer, exposed as
    `state[p]["momentum_buffer"]` from a parameter's first step on (as torch does).  `step(guard=, zero_grad=)`: guard
    is a device float that switches the update off when non-zero; zero_grad stores zeros to the gradients read.  (A
    guarded-off step still counts as a parameter's first: its momentum buffer then starts from zeros instead of the
    next gradient — the loop is about to stop on the meter's NaN warning anyway.)"""
    _NAME, _TORCH, _REFUSED = "HipSGD", "torch.optim.SGD", ("maximize", "differentiable")
    _HYP_DTYPE, _KEY_COLS = torch.float32, 5
    _build = staticmethod(build_sgd_tables)
    _launch = staticmethod(sgd_step)

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_tables()
        self._allocate([p for g in self.param_groups if g["momentum"] != 0 for p in g["params"]])

    def _allocate(self, params):
        params = [p for p in params if p not in self._slots]
        if not params:
            return
        for p, v in zip(params, self._carve([p.numel() for p in params], params[0].device)):
            self._slots[p] = v.view_as(p)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._refuse_groups()
        for g in self.param_groups:
            for p in g["params"]:
                buf = self.state.get(p, {}).get("momentum_buffer")
                if buf is None:
                    continue
                self._allocate([p])
                slot = self._slots[p]
                if buf.data_ptr() != slot.data_ptr():
                    slot.copy_(buf.to(device=slot.device, dtype=torch.float32).view_as(slot))
                    self.state[p]["momentum_buffer"] = slot
        self._invalidate()

    def _hyper_values(self):
        return tuple((float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]), float(g["dampening"]),
                      1.0 if g["nesterov"] else 0.0) for g in self.param_groups)

    def _check_hyper(self):
        for g in self.param_groups:
            if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _sig_extra(self):
        return [g["momentum"] != 0 for g in self.param_groups]

    def _entries(self):
        entries, firsts = [], []
        self._refuse_groups()
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                grad = self._checked_grad(p)
                if grad is None:
                    continue  # absent: left untouched, as torch does
                buf, first = 0, 0
                if g["momentum"] != 0:
                    if p not in self._slots:
                        self._allocate([q for q in g["params"]])
                    buf = self._slots[p].data_ptr()
                    have = self.state[p].get("momentum_buffer") if p in self.state else None
                    if have is None:
                        first = 1
                    elif have.data_ptr() != buf:  # a buffer somebody assigned by hand: adopt its values
                        self._slots[p].copy_(have)
                        self.state[p]["momentum_buffer"] = self._slots[p]
                entries.append((p.data_ptr(), grad.data_ptr(), buf, p.numel(), gi, first))
                if first:
                    firsts.append(p)
        return entries, firsts

    def _after_fresh(self, firsts):
        # the first-step flags are spent: the table in device memory says so before the next launch
        for p in firsts:
            self.state[p]["momentum_buffer"] = self._slots[p]
        self._table[:, 5] = 0
        self._table_dev = self._table.to(self._table_dev.device)


# ---------------------------------------------------------------------------------------------------------- LARS
class HipLARS(HipSGD):
    """HipSGD behind a layer-wise trust ratio — LARS / LARC (upstream SlowFast's SOLVER.LARS_ON, NVIDIA apex's LARC):

        opt = HipLARS(groups, lr=..., momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02, clip=True)
        loss.backward(); opt.step(guard=loss_fun.guard, zero_grad=True)

    Per tensor, with pn = ||p||, gn = ||g|| and the group's lr and weight decay wd:
    r = trust_coefficient * pn / (gn + pn * wd + eps), with `clip` r = min(r / lr, 1) (LARC's clipping mode: the
    step never exceeds plain SGD's); then g = (g + wd * p) * r goes through SGD's momentum and p -= lr * g.  A tensor
    with a zero norm gets r = 1 and no decay.  Groups with `apply_LARS` False (a group key, default True) and, with
    `ignore_1d_param`, one-dimensional parameters (BN scales, biases) get plain SGD with weight decay.

    `step()` is two native calls: `sf_lars_ratios` (two launches: both norms of every tensor in fp64 in a fixed order —
    equal gradients give equal bits, whatever their alignment) and `sf_lars_sgd_step` (HipSGD's launch reading {r, wd_t}
    per tensor).  Nothing is read on the host: lr, weight decay, trust_coefficient, eps and the switches live in device
    memory (`upload_hyper()` as for HipSGD, so a captured step follows the schedule), `.ratios` is a device fp32
    [n_tensors, 2] view (table order: the parameters with a gradient, group by group) and `.guard` a fixed-address
    float32 [1] that is non-zero when the `guard` handed to `step()` was raised or a parameter or gradient is not
    finite — the update launch takes it, so such a step moves nothing.  Partials, ratios and that state are views of ONE
    allocation the optimizer owns.  `state_dict()` is torch.optim.SGD's (the ratios are not state; `apply_LARS` rides
    in the param_groups, and groups loaded without it keep the value they had)."""
    _NAME = "HipLARS"

    def __init__(self, params, *args, trust_coefficient=0.02, clip=True, eps=1e-8, ignore_1d_param=False, **kwargs):
        for name, v in (("trust_coefficient", trust_coefficient), ("eps", eps)):
            f = float(v)
            if not (f >= 0.0) or f == float("inf"):
                raise ValueError("HipLARS: %s must be a finite number that is not negative, got %r" % (name, v))
        self.trust_coefficient, self.eps = float(trust_coefficient), float(eps)
        self.clip, self.ignore_1d_param = bool(clip), bool(ignore_1d_param)
        self._lars_table = self._lars_table_dev = self._lars_block = None
        self._partials = self._ratios = self._lars_state = None
        super().__init__(params, *args, **kwargs)
        self.defaults["apply_LARS"] = True
        for g in self.param_groups:
            g.setdefault("apply_LARS", True)

    def load_state_dict(self, state_dict):
        keep = [g.get("apply_LARS", True) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, a in zip(self.param_groups, keep):
            g.setdefault("apply_LARS", a)

    # ---- device memory this object owns
    def _lars_field(self, name):
        if self._lars_state is None:
            raise RuntimeError("HipLARS.%s: nothing has been computed yet — it exists from the first step() on" % name)
        return self._lars_state

    @property
    def guard(self):
        """float32 [1] on the GPU: the guard of the last step (the one handed in, or a non-finite parameter / gradient)."""
        return self._lars_field("guard")[ST_GUARD:ST_GUARD + 1]

    @property
    def nonfinite(self):
        return self._lars_field("nonfinite")[ST_FLAG:ST_FLAG + 1]

    @property
    def ratios(self):
        """fp32 [n_tensors, 2] on the GPU: {r, wd_t} of the last step, in table order."""
        self._lars_field("ratios")
        return self._ratios

    def _hyper_values(self):
        # ONE row: sf_lars_sgd_step's [n_groups][5], then sf_lars_ratios' [n_groups + 1][3] — one upload serves both
        flat = [v for row in super()._hyper_values() for v in row]
        for g in self.param_groups:
            flat += [float(g["lr"]), float(g["weight_decay"]), 1.0 if g.get("apply_LARS", True) else 0.0]
        flat += [float(self.trust_coefficient), float(self.eps), 1.0 if self.clip else 0.0]
        return (tuple(flat),)

    def _build(self, entries, chunk):
        table, chunks = build_sgd_tables(entries, chunk)
        plist = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        assert len(plist) == len(entries)
        lars = [(e[0], e[1], e[3], e[4], self.ignore_1d_param and p.dim() <= 1) for e, p in zip(entries, plist)]
        self._lars_table, lars_chunks = build_lars_tables(lars, chunk)
        assert torch.equal(lars_chunks, chunks)
        dev = plist[0].device
        self._lars_table_dev = self._lars_table.to(dev)
        n, nc = len(entries), chunks.shape[0]
        if self._partials is None or self._partials.numel() != 2 * nc or self._ratios.shape[0] != n:
            if self._lars_block is not None:
                self._blocks = [b for b in self._blocks if b is not self._lars_block]
            part, ratios, state = self._carve([4 * nc, 2 * n, CLIP_STATE], dev)
            self._lars_block = self._blocks[-1]
            self._partials, self._ratios, self._lars_state = part.view(torch.float64), ratios.view(n, 2), state
        return table, chunks

    def _launch(self, table_host, table, chunks_host, chunks, hyper_host, hyper, guard, zero_grad):
        G = len(self.param_groups)
        k = G * HYP_ROW
        lars_ratios(self._lars_table, self._lars_table_dev, chunks_host, chunks,
                    hyper_host[0, k:].view(G + 1, LARS_HYP_ROW), hyper[0, k:].view(G + 1, LARS_HYP_ROW), self._partials,
                    self._ratios, self._lars_state, guard=guard)
        lars_sgd_step(table_host, table, chunks_host, chunks, hyper_host[0, :k].view(G, HYP_ROW),
                      hyper[0, :k].view(G, HYP_ROW), self._ratios, guard=self._lars_state[ST_GUARD:ST_GUARD + 1],
                      zero_grad=zero_grad)


# ---------------------------------------------------------------------------------------------------------- Adam
class _AdamTables(_TableOptimizer):
    """What HipAdam and HipAdamW share: the state slots, their adoption from a checkpoint and the address table."""
    _HYP_DTYPE, _KEY_COLS = torch.float64, 7
    _build = staticmethod(build_adam_tables)

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        self._init_tables()
        self._allocate([p for g in self.param_groups for p in g["params"]])

    def _allocate(self, params):
        params = [p for p in params if p not in self._slots]
        if not params:
            return
        views = self._carve([k for p in params for k in (p.numel(), p.numel(), 1)], params[0].device)
        for i, p in enumerate(params):
            self._slots[p] = {"exp_avg": views[3 * i].view_as(p), "exp_avg_sq": views[3 * i + 1].view_as(p),
                              "step": views[3 * i + 2].view(())}

    def _adopt(self, p):
        """Make state[p] the owned slots, taking over the values of tensors that live elsewhere (a checkpoint's, or
        ones assigned by hand; torch's own `step` is a CPU tensor)."""
        self._allocate([p])
        st = self.state[p]
        if "max_exp_avg_sq" in st:
            raise ValueError("%s: amsgrad state (max_exp_avg_sq) is not supported — use %s" % (self._NAME, self._TORCH))
        for k, slot in self._slots[p].items():
            have = st.get(k)
            if have is None:
                raise ValueError("%s: state without %r" % (self._NAME, k))
            if not torch.is_tensor(have):
                slot.fill_(float(have))
            elif have.data_ptr() != slot.data_ptr():
                slot.copy_(have.detach().to(device=slot.device, dtype=torch.float32).view_as(slot))
            st[k] = slot

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._refuse_groups()
        for g in self.param_groups:
            for p in g["params"]:
                if len(self.state.get(p, {})) != 0:
                    self._adopt(p)
        self._invalidate()

    def _hyper_values(self):
        return tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                      float(g["weight_decay"])) for g in self.param_groups)

    def _sig_extra(self):
        return ()

    def _entries(self):
        entries, fresh = [], []
        self._refuse_groups()
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                grad = self._checked_grad(p)
                if grad is None:
                    continue  # absent: left untouched and without state, as torch does
                if p not in self._slots:
                    self._allocate([q for q in g["params"]])
                s = self._slots[p]
                if len(self.state.get(p, {})) == 0:
                    fresh.append(p)
                elif any(self.state[p].get(k) is not s[k] for k in s):
                    self._adopt(p)
                entries.append((p.data_ptr(), grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(),
                                s["step"].data_ptr(), p.numel(), gi))
        return entries, fresh

    def _after_fresh(self, fresh):
        for p in fresh:
            self.state[p].update(self._slots[p])


class HipAdam(_AdamTables, torch.optim.Adam):
    """torch.optim.Adam (same constructor, param_groups and state_dict keys) whose `step()` is ONE native call over every
    parameter of every group (`sf_adam_step`).

    `exp_avg`, `exp_avg_sq` and `step` are 16-byte aligned views of one allocation owned by the optimizer; `step` is a
    float32 scalar in DEVICE memory per parameter (torch keeps it on the host), advanced by the call itself, so a
    captured step keeps counting when it is replayed.  They appear in `state[p]` from the parameter's first step on;
    a parameter whose `.grad` is None is left untouched and gets no state.  `step(guard=, zero_grad=)` as in HipSGD: a
    guarded-off step moves nothing — parameters, moments, step counts, gradients."""
    _NAME, _TORCH = "HipAdam", "torch.optim.Adam"
    _REFUSED = ("amsgrad", "maximize", "differentiable", "decoupled_weight_decay")
    _launch = staticmethod(adam_step)


class HipAdamW(_AdamTables, torch.optim.AdamW):
    """torch.optim.AdamW (same constructor, param_groups and state_dict keys) the way HipAdam is torch.optim.Adam: ONE
    native call (`sf_adamw_step`, HipAdam's kernel body with the decay decoupled — p *= 1 - lr * weight_decay in front of
    the update, nothing added to the gradient).  State layout, guard, zero_grad, checkpoints and stream capture are
    HipAdam's; a state dict saved by torch.optim.AdamW loads, and the reverse.  Groups with `decoupled_weight_decay`
    switched off are refused: that is HipAdam."""
    _NAME, _TORCH = "HipAdamW", "torch.optim.AdamW"
    _REFUSED = ("amsgrad", "maximize", "differentiable")
    _launch = staticmethod(adamw_step)

    def _refuse_groups(self):
        super()._refuse_groups()
        for g in self.param_groups:
            if not g.get("decoupled_weight_decay", True):
                raise ValueError("HipAdamW: decoupled_weight_decay = False is torch.optim.Adam's update — use HipAdam")


# ------------------------------------------------------------------------------------------------ gradient clipping
CLIP_TAB_ROW = 2                                              # gradient address, numel
CLIP_STATE = 8                                                # floats of the state block sf_grad_norm writes
ST_NORM32, ST_COEF, ST_FLAG, ST_GUARD = 2, 3, 4, 5            # its fields ([0..1]: the norm as one fp64)
NORM_INF, NORM_L2 = 0, 2                                      # SF_NORM_INF, SF_NORM_L2
ROW_GRAD_NORM = 7                                             # the ring column sf_grad_norm fills


def build_clip_tables(entries, chunk):
    """entries: (gradient address, numel) per tensor -> (table int64 [n, 2], chunks int64 [n_chunks, 2]), tiled as
    build_sgd_tables does."""
    return _build_tables(entries, chunk, CLIP_TAB_ROW, 1)


def _clip_tables_args(tag, table_host, table, chunks_host, chunks):
    args = _tables_args(tag, table_host, table, chunks_host, chunks)
    if not (table.is_cuda and chunks.is_cuda):
        raise sfhip.SfhipError("%s: table and chunks live on the GPU — there is no CPU fallback" % tag)
    return args


def grad_norm(table_host, table, chunks_host, chunks, norm_type, partials, state, max_norm=None, guard=None, ring=None):
    """One `sf_grad_norm` call (two launches): the total norm of the gradients in the table into `state` (fp32 [8]: the
    norm as fp64 in [0:2], then norm, coefficient, non-finite flag, guard_out).  partials fp64 [n_chunks]; max_norm a
    device fp32 [1] or None; guard the loss's guard or None; ring a StatsRing or None."""
    args = _clip_tables_args("grad_norm", table_host, table, chunks_host, chunks)
    if not (partials.is_cuda and state.is_cuda):
        raise sfhip.SfhipError("grad_norm: partials and state live on the GPU — there is no CPU fallback")
    assert partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() >= chunks_host.shape[0]
    assert state.dtype == torch.float32 and state.is_contiguous() and state.numel() >= CLIP_STATE
    sfhip._call("sf_grad_norm", *args, int(norm_type), _vp(max_norm), _vp(guard), _vp(partials), _vp(state),
                *_ring_args(ring), tag="grad_norm")


def grad_scale(table_host, table, chunks_host, chunks, state):
    """One `sf_grad_scale` launch: g *= state[3], nothing touched when state[5] (the guard) is raised or state[3] is 1."""
    args = _clip_tables_args("grad_scale", table_host, table, chunks_host, chunks)
    if not state.is_cuda:
        raise sfhip.SfhipError("grad_scale: state lives on the GPU — there is no CPU fallback")
    sfhip._call("sf_grad_scale", *args, _vp(state), tag="grad_scale")


def grad_clamp(table_host, table, chunks_host, chunks, value):
    """One `sf_grad_clamp` launch: g = clamp(g, -value, value), value a device fp32 [1]."""
    args = _clip_tables_args("grad_clamp", table_host, table, chunks_host, chunks)
    if not value.is_cuda:
        raise sfhip.SfhipError("grad_clamp: value lives on the GPU — there is no CPU fallback")
    sfhip._call("sf_grad_clamp", *args, _vp(value), tag="grad_clamp")


def _positive_or_none(v, name):
    if v is None:
        return None
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError("HipGradClip: %s must be a positive finite number, got %r" % (name, v))
    if not (f > 0.0) or f == float("inf"):
        raise ValueError("HipGradClip: %s must be a positive finite number, got %r" % (name, v))
    return f


class HipGradClip(object):
    """`torch.nn.utils.clip_grad_norm_` / `clip_grad_value_` between `loss.backward()` and `optimizer.step()`, on
    libsfhip kernels over an address table of every gradient (`sf_grad_clamp`, `sf_grad_norm`, `sf_grad_scale`):

        clip = HipGradClip(optimizer.param_groups, max_norm=1.0, ring=meter.ring)
        loss.backward(); clip.clip(guard=loss_fun.guard); optimizer.step(guard=clip.guard)

    `parameters` is an iterable of parameters or an optimizer's `param_groups`; parameters whose `.grad` is None are
    skipped, as torch does.  `clip(guard=None)` clamps to [-clip_value, clip_value] (if `clip_value`), then computes the
    total norm (`norm_type` 2 or inf) and scales by min(1, max_norm / (norm + 1e-6)) (if `max_norm`) — the order
    upstream SlowFast applies when both SOLVER.CLIP_GRAD_VAL and SOLVER.CLIP_GRAD_L2NORM are set.  The norm is summed
    in fp64 in a fixed order (equal gradients give equal bits); the scale launch touches no memory when the
    coefficient is exactly 1.  Nothing is read on the host: `max_norm` / `clip_value` live in device memory (assign the
    attributes; `clip()` / `upload_hyper()` turn a change into one small copy), `.total_norm` is a device fp32 view,
    `.guard` a fixed-address float32 [1] that is non-zero when the `guard` handed to `clip()` was raised or a gradient
    is not finite — hand it to `optimizer.step(guard=clip.guard)`.  With `ring` (the meter's StatsRing) the norm goes
    to column 7 of the row the step's loss kernel wrote (`DeviceTrainMeter(grad_norm=True)` logs it).

    One deviation from torch: when the norm is not finite the gradients are left EXACTLY as they are and the guard is
    raised; torch multiplies every gradient by NaN.  Either way the step is lost — here the parameters survive (the
    guarded optimizer skips the update) and the meter reports it.

    With `clip_value` alone no norm pass runs, so there is nothing to put behind `.guard` / `.total_norm`: they raise
    then — hand the loss's guard to the optimizer.  Under stream capture `clip()` refuses to build a new address table:
    warm up eagerly first.  An empty parameter list, or one without gradients, is a no-op without a launch.  There is no
    fallback: gradients that are not contiguous fp32 tensors on the current GPU are refused."""

    def __init__(self, parameters, max_norm=None, norm_type=2.0, clip_value=None, ring=None):
        params = []
        for p in parameters:
            params += list(p["params"]) if isinstance(p, dict) else [p]
        for p in params:
            if not torch.is_tensor(p):
                raise ValueError("HipGradClip: parameters are tensors or param_groups, got %s" % type(p).__name__)
        try:
            nt = float(norm_type)
        except (TypeError, ValueError):
            nt = None
        if nt not in (2.0, float("inf")):
            raise ValueError("HipGradClip: norm_type must be 2 or inf, got %r" % (norm_type,))
        self.norm_type = nt
        self.max_norm = _positive_or_none(max_norm, "max_norm")
        self.clip_value = _positive_or_none(clip_value, "clip_value")
        if self.max_norm is None and self.clip_value is None:
            raise ValueError("HipGradClip: give max_norm, clip_value or both")
        self._modes = (self.max_norm is not None, self.clip_value is not None)
        self.ring = ring
        self._params = params
        self._sig = None
        self._table = self._chunks = self._table_dev = self._chunks_dev = self._partials = None
        self._state = self._hyper_dev = self._hyper_vals = None
        self._stage = _HyperStage()

    # ---- device memory this object owns
    def _device(self):
        for p in self._params:
            if p.is_cuda:
                return p.device
        raise sfhip.SfhipError("HipGradClip: no parameter is on a GPU — the clipping kernels run on the GPU only "
                               "(no CPU fallback)")

    def _ensure_state(self):
        if self._state is None:
            self._state = torch.zeros((CLIP_STATE,), dtype=torch.float32, device=self._device())
            self._state[ST_COEF] = 1.0
        return self._state

    def _norm_field(self, name, i):
        if self.max_norm is None:
            raise RuntimeError("HipGradClip.%s: no norm pass runs with clip_value alone — hand the loss's guard to the "
                               "optimizer" % name)
        return self._ensure_state()[i:i + 1]

    guard = property(lambda self: self._norm_field("guard", ST_GUARD))
    total_norm = property(lambda self: self._norm_field("total_norm", ST_NORM32))
    coef = property(lambda self: self._norm_field("coef", ST_COEF))
    nonfinite = property(lambda self: self._norm_field("nonfinite", ST_FLAG))

    @property
    def total_norm64(self):
        """The norm as the kernel summed it: a device fp64 [1] view."""
        self._norm_field("total_norm64", 0)
        return self._state[0:2].view(torch.float64)

    def upload_hyper(self):
        """Copy max_norm / clip_value to the device if they changed since the last upload (HipSGD.upload_hyper's way:
        a pinned staging row, one small copy on the current stream).  Call it before replaying a captured `clip()`
        after assigning either attribute.  Returns whether anything was copied."""
        self.max_norm = _positive_or_none(self.max_norm, "max_norm")
        self.clip_value = _positive_or_none(self.clip_value, "clip_value")
        vals = (self.max_norm, self.clip_value)
        if vals == self._hyper_vals:
            return False
        if tuple(v is not None for v in vals) != self._modes:
            raise ValueError("HipGradClip: max_norm / clip_value cannot be switched on or off after construction")
        row = torch.tensor([v if v is not None else 0.0 for v in vals], dtype=torch.float32)
        if self._hyper_dev is None:
            self._hyper_dev = torch.empty((2,), dtype=torch.float32, device=self._device())
        self._stage.upload(row, self._hyper_dev)
        self._hyper_vals = vals
        return True

    # ---- the address table
    @staticmethod
    def _checked_grad(p):
        g = p.grad
        if g is None:
            return None
        if g.dtype != torch.float32:  # (sparse ones: refused by _signature)
            raise ValueError("HipGradClip: gradient of dtype %s — float32 only" % g.dtype)
        if not g.is_contiguous():
            raise ValueError("HipGradClip: gradients must be contiguous")
        sfhip._require_gpu(g, "HipGradClip")
        return g if g.numel() > 0 else None

    def _signature(self):
        grads = [p.grad for p in self._params]
        if any(g is not None and g.is_sparse for g in grads):  # (a sparse tensor has no address to sign with)
            raise ValueError("HipGradClip: sparse gradients are not supported — use torch.nn.utils.clip_grad_norm_")
        return [0 if g is None else g.data_ptr() for g in grads]

    def _rebuild(self):
        entries = []
        for p in self._params:
            g = self._checked_grad(p)
            if g is not None:
                entries.append((g.data_ptr(), g.numel()))
        if not entries:
            self._table = None
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("HipGradClip.clip under stream capture needs a new address table, which takes "
                               "host-to-device copies — warm up eagerly first (run the same step outside the capture)")
        dev = self._device()
        self._table, self._chunks = build_clip_tables(entries, sfhip.lib().sf_sgd_chunk_elems())
        self._table_dev, self._chunks_dev = self._table.to(dev), self._chunks.to(dev)
        if self._partials is None or self._partials.numel() < self._chunks.shape[0]:
            self._partials = torch.zeros((self._chunks.shape[0],), dtype=torch.float64, device=dev)

    @torch.no_grad()
    def clip(self, guard=None):
        """Clamp, then norm + scale, as configured; `guard` is the loss's guard (a float32 tensor on the GPU) or None.
        Returns `.total_norm` (a device view, not a host number) when a norm pass ran, else None."""
        if not self._params:
            return None
        sig = self._signature()
        if sig != self._sig:
            self._rebuild()
            self._sig = sig
        if self._table is None:
            return None
        if not torch.cuda.is_current_stream_capturing():
            self.upload_hyper()
        elif self._hyper_dev is None:
            raise RuntimeError("HipGradClip.clip under stream capture: warm up eagerly first")
        if guard is not None and (not guard.is_cuda or guard.dtype != torch.float32):
            raise ValueError("HipGradClip.clip: guard is a float32 tensor on the GPU")
        tabs = (self._table, self._table_dev, self._chunks, self._chunks_dev)
        if self.clip_value is not None:
            grad_clamp(*tabs, self._hyper_dev[1:2])
        if self.max_norm is None:
            return None
        state = self._ensure_state()
        grad_norm(*tabs, NORM_L2 if self.norm_type == 2.0 else NORM_INF, self._partials, state,
                  max_norm=self._hyper_dev[0:1], guard=guard, ring=self.ring)
        grad_scale(*tabs, state)
        return state[ST_NORM32:ST_NORM32 + 1]


def construct_hip_grad_clip(model, cfg, ring=None):
    """Upstream SlowFast's SOLVER.CLIP_GRAD_L2NORM / SOLVER.CLIP_GRAD_VAL as a HipGradClip over the model's parameters,
    or None when the config has neither key or both are None (config/defaults.py mirrors the reference's key set, which
    has neither: set them with `cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0` on a config that allows new keys, or build the
    HipGradClip directly)."""
    max_norm = cfg.SOLVER.get("CLIP_GRAD_L2NORM", None)
    clip_value = cfg.SOLVER.get("CLIP_GRAD_VAL", None)
    if max_norm is None and clip_value is None:
        return None
    return HipGradClip(model.parameters(), max_norm=max_norm, norm_type=2.0, clip_value=clip_value, ring=ring)


def _split_bn_params(model, cfg):
    """models/optimizer.py:26-51: BatchNorm parameters ("bn" in the name) get BN.WEIGHT_DECAY, the rest
    SOLVER.WEIGHT_DECAY."""
    bn_params, non_bn_parameters = [], []
    for name, p in model.named_parameters():
        (bn_params if "bn" in name else non_bn_parameters).append(p)
    optim_params = [{"params": bn_params, "weight_decay": cfg.BN.WEIGHT_DECAY},
                    {"params": non_bn_parameters, "weight_decay": cfg.SOLVER.WEIGHT_DECAY}]
    assert len(list(model.parameters())) == len(non_bn_parameters) + len(bn_params), \
        "parameter size does not match: {} + {} != {}".format(len(non_bn_parameters), len(bn_params),
                                                              len(list(model.parameters())))
    return optim_params


def construct_hip_optimizer(model, cfg):
    """models/optimizer.py:26-58 for SOLVER.OPTIMIZING_METHOD == "sgd" (a HipSGD).  "adam" keeps raising here, as it
    always has — its branch of the reference (:59-65) is `construct_hip_adam`, and `construct_hip_solver` picks
    between the two by name."""
    optim_params = _split_bn_params(model, cfg)
    if cfg.SOLVER.OPTIMIZING_METHOD == "sgd":
        return HipSGD(optim_params, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM,
                      weight_decay=cfg.SOLVER.WEIGHT_DECAY, dampening=cfg.SOLVER.DAMPENING,
                      nesterov=cfg.SOLVER.NESTEROV)
    if cfg.SOLVER.OPTIMIZING_METHOD == "adam":
        raise NotImplementedError("construct_hip_optimizer builds sgd only; for 'adam' call construct_hip_adam(model, "
                                  "cfg) or construct_hip_solver(model, cfg): a HipAdam, torch.optim.Adam's subclass "
                                  "(the reference's models/optimizer.py:59-65)")
    raise NotImplementedError("Does not support {} optimizer".format(cfg.SOLVER.OPTIMIZING_METHOD))


def construct_hip_adam(model, cfg):
    """models/optimizer.py:59-65: torch.optim.Adam(betas=(0.9, 0.999)) over the same parameter split, as a HipAdam."""
    return HipAdam(_split_bn_params(model, cfg), lr=cfg.SOLVER.BASE_LR, betas=(0.9, 0.999),
                   weight_decay=cfg.SOLVER.WEIGHT_DECAY)


def construct_hip_adamw(model, cfg):
    """Upstream SlowFast's SOLVER.OPTIMIZING_METHOD == "adamw": torch.optim.AdamW(betas=(0.9, 0.999)) over the same
    parameter split, as a HipAdamW."""
    return HipAdamW(_split_bn_params(model, cfg), lr=cfg.SOLVER.BASE_LR, betas=(0.9, 0.999),
                    weight_decay=cfg.SOLVER.WEIGHT_DECAY)


def _lars_keys(cfg):
    """Upstream SlowFast's SOLVER.LARS_ON read with `.get` (config/defaults.py mirrors the reference's key set, which
    has no such key: set it on a config that allows new keys) -> (on, trust_coefficient, clip).  Upstream wraps its SGD
    as LARS(optimizer, trust_coefficient=0.001, clip=False); SOLVER.LARS_TRUST_COEFFICIENT / SOLVER.LARS_CLIP, where a
    config has them, replace those two."""
    node = cfg.SOLVER
    return (bool(node.get("LARS_ON", False)), float(node.get("LARS_TRUST_COEFFICIENT", 0.001)),
            bool(node.get("LARS_CLIP", False)))


def construct_hip_lars(model, cfg):
    """SOLVER.OPTIMIZING_METHOD == "sgd" with upstream's SOLVER.LARS_ON: construct_hip_optimizer's SGD as a HipLARS.  The
    BatchNorm group does not apply LARS (plain SGD with BN.WEIGHT_DECAY), the rest does."""
    _, trust, clip = _lars_keys(cfg)
    groups = _split_bn_params(model, cfg)
    groups[0]["apply_LARS"] = False
    return HipLARS(groups, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM, weight_decay=cfg.SOLVER.WEIGHT_DECAY,
                   dampening=cfg.SOLVER.DAMPENING, nesterov=cfg.SOLVER.NESTEROV, trust_coefficient=trust, clip=clip)


def construct_hip_solver(model, cfg):
    """models/optimizer.py:26-69 whole: "sgd" -> HipSGD (with upstream's SOLVER.LARS_ON: HipLARS), "adam" -> HipAdam,
    upstream's "adamw" -> HipAdamW, anything else raises the reference's NotImplementedError."""
    if cfg.SOLVER.OPTIMIZING_METHOD == "adam":
        return construct_hip_adam(model, cfg)
    if cfg.SOLVER.OPTIMIZING_METHOD == "adamw":
        return construct_hip_adamw(model, cfg)
    if cfg.SOLVER.OPTIMIZING_METHOD == "sgd" and _lars_keys(cfg)[0]:
        return construct_hip_lars(model, cfg)
    return construct_hip_optimizer(model, cfg)
