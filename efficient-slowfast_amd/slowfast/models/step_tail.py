"""The training iteration behind the backward pass (reference tools/train_net.py:67-157) on libsfhip kernels.

* `StatsRing` — device memory the loss kernel writes one row of statistics into per step (loss, top-1 / top-k error,
  non-finite flag, batch size, bad-label count); `utils.meters.DeviceTrainMeter` drains it once per LOG_PERIOD.
* `HipCrossEntropy(topk, ring)` — `loss_fun(preds, labels)` of train_net.py:84-87, `misc.check_nan_losses` (:90) and
  `metrics.topks_correct` (:122-125) as ONE launch (`sf_ce_topk`) with no host read.
* `HipSGD` — `torch.optim.SGD` whose `step()` is ONE launch over every parameter of every group (`sf_sgd_step`), with the
  hyper-parameters in device memory: `optim.set_lr` (:68-69) stays a host assignment, `step()` / `upload_hyper()` turn a
  change into one small copy, and a captured step follows the schedule.
* `construct_hip_optimizer(model, cfg)` — models/optimizer.py:26-58 for `sgd`.
There is no fallback: tensors that are not fp32 on the current GPU are refused."""
import ctypes

import torch

import sfhip

RING_ROW = 8
TAB_ROW, HYP_ROW = 6, 5
STAGE_SLOTS = 16
ROW_LOSS, ROW_TOP1, ROW_TOPK, ROW_FLAG, ROW_N, ROW_BAD = 0, 1, 2, 3, 4, 5


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


def ce_topk(preds, labels, k_hi, ring, out, dlogits=None):
    """One `sf_ce_topk` launch.  preds fp32 [N, K] (unit column stride, row stride >= K), labels int64 [N], out fp32 [2]
    (loss, non-finite flag).  Returns dlogits [N, K]."""
    sfhip._require_gpu(preds, "ce_topk")
    if preds.dim() != 2 or labels.dim() != 1 or labels.shape[0] != preds.shape[0]:
        raise ValueError("ce_topk: preds [N, K] and labels [N], got %s and %s" % (tuple(preds.shape), tuple(labels.shape)))
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise ValueError("ce_topk: labels must be int64 on the GPU, got %s on %s" % (labels.dtype, labels.device))
    N, K = preds.shape
    if N > 0 and K > 0 and (preds.stride(1) != 1 or (N > 1 and preds.stride(0) < K)):
        preds = preds.contiguous()
    ld = preds.stride(0) if N > 1 else K
    labels = labels.contiguous()
    if dlogits is None:
        dlogits = torch.empty((N, K), dtype=torch.float32, device=preds.device)
    assert dlogits.is_contiguous() and tuple(dlogits.shape) == (N, K) and out.numel() >= 2
    cnt = ctypes.cast(ctypes.c_void_p(ring.counter.data_ptr()), sfhip._pi)
    sfhip._call("sf_ce_topk", _vp(preds), int(ld), _vp(labels), N, K, int(k_hi), _vp(dlogits), _vp(ring.rows), cnt,
                ring.cap, _vp(out), tag="ce_topk")
    return dlogits


class _CEFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, labels, owner):
        d = ce_topk(preds.detach(), labels, owner.topk, owner.ring, owner.out)
        owner.dlogits = d
        ctx.save_for_backward(d)
        return owner.out[0].clone() if owner.keep_loss else owner.out[0]

    @staticmethod
    def backward(ctx, grad_output):
        (d,) = ctx.saved_tensors
        return d * grad_output, None, None


class HipCrossEntropy(object):
    """`loss = HipCrossEntropy(cfg.TRAIN.TOPK, ring)(preds, labels)`; `loss.backward()` as in the reference, or
    `.backward_direct(preds)` to hand the stored gradient to autograd without the multiply by grad_output (= 1).
    `guard` is the step's non-finite flag at a fixed address: `HipSGD.step(guard=loss_fun.guard)`.  The returned loss
    is a view of a buffer the next call overwrites (keep_loss=True returns a copy, one more launch)."""

    def __init__(self, topk, ring, keep_loss=False):
        if int(topk) < 1:
            raise ValueError("HipCrossEntropy: topk must be at least 1, got %r" % (topk,))
        self.topk, self.ring, self.keep_loss = int(topk), ring, bool(keep_loss)
        self.out = torch.zeros((2,), dtype=torch.float32, device=ring.rows.device)
        self.dlogits = None

    @property
    def guard(self):
        return self.out[1:2]

    def __call__(self, preds, labels):
        return _CEFunction.apply(preds, labels, self)

    def backward_direct(self, preds):
        if self.dlogits is None or tuple(self.dlogits.shape) != tuple(preds.shape):
            raise RuntimeError("HipCrossEntropy.backward_direct: call the loss on these predictions first")
        preds.backward(gradient=self.dlogits)


# ---------------------------------------------------------------------------------------------------------- SGD
def build_sgd_tables(entries, chunk):
    """entries: (parameter address, gradient address, momentum address, numel, group, first) per tensor ->
    (table int64 [n, 6], chunks int64 [n_chunks, 2]): a chunk is (tensor index, first element) and covers at most
    `chunk` elements of one tensor; the chunks tile the tensors in order."""
    table = torch.tensor([list(map(int, e)) for e in entries], dtype=torch.int64).reshape(-1, TAB_ROW)
    rows = []
    for i, e in enumerate(entries):
        rows += [(i, s) for s in range(0, int(e[3]), chunk)]
    return table, torch.tensor(rows, dtype=torch.int64).reshape(-1, 2)


def sgd_step(table_host, table, chunks_host, chunks, hyper_host, hyper, guard=None, zero_grad=False):
    """One `sf_sgd_step` launch; the host tensors are what the device ones were uploaded from."""
    for h, d in ((table_host, table), (chunks_host, chunks)):
        assert h.dtype == d.dtype == torch.int64 and h.is_contiguous() and d.is_contiguous() and not h.is_cuda
        assert h.shape == d.shape
    assert hyper_host.dtype == hyper.dtype == torch.float32 and hyper_host.shape == hyper.shape and hyper.is_contiguous()
    if not (table.is_cuda and chunks.is_cuda and hyper.is_cuda):
        raise sfhip.SfhipError("sgd_step: table, chunks and hyper live on the GPU — there is no CPU fallback")
    sfhip._call("sf_sgd_step", _vp(table_host), _vp(table), table_host.shape[0], _vp(chunks_host), _vp(chunks),
                chunks_host.shape[0], _vp(hyper_host), _vp(hyper), hyper_host.shape[0], _vp(guard),
                1 if zero_grad else 0, tag="sgd_step")


class HipSGD(torch.optim.SGD):
    """torch.optim.SGD (same constructor, param_groups and state_dict) with a one-launch `step()`.

    Momentum buffers are 16-byte aligned views of one allocation owned by the optimizer, exposed as
    `state[p]["momentum_buffer"]` from a parameter's first step on (as torch does).  `step(guard=, zero_grad=)`: guard
    is a device float that switches the update off when non-zero; zero_grad stores zeros to the gradients read.  (A
    guarded-off step still counts as a parameter's first: its momentum buffer then starts from zeros instead of the
    next gradient — the loop is about to stop on the meter's NaN warning anyway.)"""

    def __init__(self, params, *args, **kwargs):
        super().__init__(params, *args, **kwargs)
        for g in self.param_groups:
            if g.get("maximize") or g.get("differentiable"):
                raise ValueError("HipSGD: maximize / differentiable are not supported — use torch.optim.SGD")
        self._slots = {}          # parameter -> its view of a momentum allocation
        self._blocks = []         # the allocations (one, unless groups or momentum were added later)
        self._key = None
        self._table = self._chunks = self._table_dev = self._chunks_dev = None
        self._hyper = self._hyper_dev = self._hyper_vals = None
        self._stage = None        # pinned staging rows of the hyper-parameter uploads
        self._sig = self._plist = None  # what the table was built from; the flat parameter list
        self._check_params()
        self._allocate([p for g in self.param_groups if g["momentum"] != 0 for p in g["params"]])

    # ---- construction-time checks and momentum storage
    def _check_params(self):
        for g in self.param_groups:
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise ValueError("HipSGD: parameter of dtype %s — float32 only" % p.dtype)
                if not p.is_contiguous():
                    raise ValueError("HipSGD: parameters must be contiguous")

    def _allocate(self, params):
        params = [p for p in params if p not in self._slots]
        if not params:
            return
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4  # every buffer starts on 16 bytes
        block = torch.zeros((n,), dtype=torch.float32, device=params[0].device)
        self._blocks.append(block)
        for p, o in zip(params, offs):
            self._slots[p] = block[o:o + p.numel()].view_as(p)

    def add_param_group(self, group):
        super().add_param_group(group)
        if hasattr(self, "_slots"):
            self._check_params()
            self._key = self._sig = self._plist = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if g.get("maximize") or g.get("differentiable"):
                raise ValueError("HipSGD: maximize / differentiable are not supported — use torch.optim.SGD")
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
        self._key = self._sig = self._plist = None

    # ---- hyper-parameters in device memory
    def _hyper_values(self):
        return tuple((float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]), float(g["dampening"]),
                      1.0 if g["nesterov"] else 0.0) for g in self.param_groups)

    def upload_hyper(self):
        """Copy the groups' lr / weight_decay / momentum / dampening / nesterov to the device if they changed since the
        last upload: one small copy on the current stream from a pinned staging row, so the host does not wait for
        the work already queued there.  Call it before `engine.replay(graph)`: a replayed step reads the values from
        device memory.  Returns whether anything was copied."""
        vals = self._hyper_values()
        if vals == self._hyper_vals:
            return False
        for g in self.param_groups:
            if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        rows = torch.tensor(vals, dtype=torch.float32).reshape(-1, HYP_ROW)
        dev = self.param_groups[0]["params"][0].device
        if self._hyper_dev is None or self._hyper_dev.shape != rows.shape:
            self._hyper_dev = torch.empty(rows.shape, dtype=torch.float32, device=dev)
        # the copy reads the staging row when the stream gets there, not now: every upload takes the next of STAGE_SLOTS
        # pinned rows and leaves an event behind it, and a row is written again only after its event has passed (the
        # host would have to run STAGE_SLOTS learning rates ahead of the device to wait here)
        if self._stage is None or self._stage.shape[1:] != rows.shape:
            self._stage = torch.empty((STAGE_SLOTS,) + tuple(rows.shape), dtype=torch.float32).pin_memory()
            self._stage_events, self._stage_next = [None] * STAGE_SLOTS, 0
        i = self._stage_next
        self._stage_next = (i + 1) % STAGE_SLOTS
        if self._stage_events[i] is not None:
            self._stage_events[i].synchronize()
        self._stage[i].copy_(rows)
        self._hyper_dev.copy_(self._stage[i], non_blocking=True)
        self._stage_events[i] = torch.cuda.Event()
        self._stage_events[i].record()
        self._hyper, self._hyper_vals = rows, vals
        return True

    # ---- the step
    def _entries(self):
        entries, firsts = [], []
        for gi, g in enumerate(self.param_groups):
            if g.get("maximize") or g.get("differentiable"):
                raise ValueError("HipSGD: maximize / differentiable are not supported — use torch.optim.SGD")
            for p in g["params"]:
                if p.grad is None:
                    continue  # absent: left untouched, as torch does
                if not p.is_cuda:
                    raise ValueError("HipSGD: parameter on %s — the update kernel runs on the GPU only" % p.device)
                if p.grad.is_sparse:
                    raise ValueError("HipSGD: sparse gradients are not supported — use torch.optim.SGD")
                if p.grad.dtype != torch.float32 or not p.grad.is_cuda or not p.grad.is_contiguous():
                    raise ValueError("HipSGD: gradients must be contiguous float32 tensors on the GPU")
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
                entries.append((p.data_ptr(), p.grad.data_ptr(), buf, p.numel(), gi, first))
                if first:
                    firsts.append(p)
        return entries, firsts

    def _signature(self):
        """What the address table depends on, cheaply: every parameter's and gradient's address, which groups have
        momentum and how many parameters have state.  Equal to the signature the table was built from = the table
        still holds (a momentum buffer re-assigned by hand is only seen at the next rebuild; load_state_dict and
        add_param_group force one)."""
        plist = self._plist
        if plist is None:
            plist = self._plist = [p for g in self.param_groups for p in g["params"]]
        grads = [p.grad for p in plist]
        return ([p.data_ptr() for p in plist], [0 if g is None else g.data_ptr() for g in grads],
                [g["momentum"] != 0 for g in self.param_groups], len(self.state))

    @torch.no_grad()
    def step(self, closure=None, guard=None, zero_grad=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sig = self._signature()
        if sig != self._sig:  # first call, or an address / a group changed: check everything and rebuild the table
            entries, firsts = self._entries()
            if not entries:
                return loss
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HipSGD.step under stream capture needs a new address table or a first momentum "
                                   "step, which take host-to-device copies — warm up eagerly first (run the same step "
                                   "outside the capture until every parameter has had one)")
            key = tuple(e[:5] for e in entries)
            self._table, chunks = build_sgd_tables(entries, sfhip.lib().sf_sgd_chunk_elems())
            dev = self.param_groups[0]["params"][0].device
            self._table_dev = self._table.to(dev)
            if key != self._key:
                self._chunks, self._chunks_dev = chunks, chunks.to(dev)
            self._key = key
        else:
            firsts = ()
        if not torch.cuda.is_current_stream_capturing():
            self.upload_hyper()
        elif self._hyper_dev is None:
            raise RuntimeError("HipSGD.step under stream capture: warm up eagerly first")
        if guard is not None and (not guard.is_cuda or guard.dtype != torch.float32):
            raise ValueError("HipSGD.step: guard is a float32 tensor on the GPU")
        sgd_step(self._table, self._table_dev, self._chunks, self._chunks_dev, self._hyper, self._hyper_dev, guard,
                 zero_grad)
        if firsts:  # the first-step flags are spent: the table in device memory says so before the next launch
            for p in firsts:
                self.state[p]["momentum_buffer"] = self._slots[p]
            self._table[:, 5] = 0
            self._table_dev = self._table.to(self._table_dev.device)
            sig = self._signature()  # the state grew
        self._sig = sig
        return loss


def construct_hip_optimizer(model, cfg):
    """models/optimizer.py:26-58 for SOLVER.OPTIMIZING_METHOD == "sgd": BatchNorm parameters ("bn" in the name) get
    BN.WEIGHT_DECAY, the rest SOLVER.WEIGHT_DECAY."""
    bn_params, non_bn_parameters = [], []
    for name, p in model.named_parameters():
        (bn_params if "bn" in name else non_bn_parameters).append(p)
    optim_params = [{"params": bn_params, "weight_decay": cfg.BN.WEIGHT_DECAY},
                    {"params": non_bn_parameters, "weight_decay": cfg.SOLVER.WEIGHT_DECAY}]
    assert len(list(model.parameters())) == len(non_bn_parameters) + len(bn_params), \
        "parameter size does not match: {} + {} != {}".format(len(non_bn_parameters), len(bn_params),
                                                              len(list(model.parameters())))
    if cfg.SOLVER.OPTIMIZING_METHOD == "sgd":
        return HipSGD(optim_params, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.MOMENTUM,
                      weight_decay=cfg.SOLVER.WEIGHT_DECAY, dampening=cfg.SOLVER.DAMPENING,
                      nesterov=cfg.SOLVER.NESTEROV)
    raise NotImplementedError("construct_hip_optimizer supports sgd only; for {!r} build torch's optimizer "
                              "(torch.optim.Adam, the reference's models/optimizer.py)".format(
                                  cfg.SOLVER.OPTIMIZING_METHOD))
