"""A second, averaged copy of the weights on libsfhip kernels (csrc/weight_avg.hip): the EMA of parameters and BN buffers
that large-batch recipes evaluate and checkpoint, or the equal-weight mean of SWA.

* `build_avg_tables`, `avg_update`, `avg_exchange` — the address table of {average, source} pairs and the two native
  calls over it (`sf_avg_update`: one launch plus the one-thread launch that advances the device-side count;
  `sf_avg_exchange`: one launch).
* `HipAveragedModel(model, decay=None, use_buffers=True)` — `torch.optim.swa_utils.AveragedModel` without the second
  module: the averages are flat views of one allocation, `update_parameters()` is ONE native call behind the
  optimizer's, and evaluation swaps the averages INTO the model (`swap()`, `applied()`), so the eval forward runs
  through the model's own packed weights, bf16 planes and folded-BN caches.
* `construct_hip_ema(model, cfg)` — SOLVER.EMA_ON / EMA_DECAY / EMA_USE_BUFFERS read with `.get`.
There is no fallback: tables that are not on the current GPU are refused."""
import contextlib
from collections import OrderedDict
from itertools import chain

import torch

import sfhip

from . import engine
from .step_tail import _HyperStage, _build_tables, _tables_args, _vp, carve_views

AVG_TAB_ROW = 4                                 # average address, source address, numel, kind
KIND_AVG, KIND_COPY, KIND_WORDS = 0, 1, 2       # float32 averaged / float32 copied / int64 words copied
MODE_EMA, MODE_MEAN, MODE_RUNNING = 0, 1, 2     # lerp by hyper[0] / lerp by 1 / (count + 1) / a + (s - a) / (count + 1)
OP_SWAP, OP_TO_SOURCE, OP_FROM_SOURCE = 0, 1, 2


def build_avg_tables(entries, chunk):
    """entries: (average address, source address, numel, kind) per tensor -> (table int64 [n, 4], chunks int64
    [n_chunks, 2]), tiled as build_sgd_tables does; the numel of a kind-2 row counts 8-byte words."""
    return _build_tables(entries, chunk, AVG_TAB_ROW, 2)


def _avg_tables_args(tag, table_host, table, chunks_host, chunks, *more):
    args = _tables_args(tag, table_host, table, chunks_host, chunks)
    if not (table.is_cuda and chunks.is_cuda and all(t is None or t.is_cuda for t in more)):
        raise sfhip.SfhipError("%s: table, chunks, count, hyper and guard live on the GPU — there is no CPU fallback" % tag)
    return args


def avg_update(table_host, table, chunks_host, chunks, mode, count, hyper_host=None, hyper=None, guard=None):
    """One `sf_avg_update` call (two launches): every kind-0 pair of the table averaged by `mode` (0: lerp by hyper[0] =
    1 - decay; 1: lerp by 1 / (count + 1); 2: a + (s - a) / (count + 1) as torch's GPU kernels round it), kinds 1 and 2
    copied, then count += 1.  count: int64 [1] (or 0-d) on the GPU; hyper / hyper_host: fp32 [1] on the GPU and the host
    value it was uploaded from (mode 0); guard: the loss's, clipper's or LARS's guard or None — raised, nothing moves,
    the count included.  The first update (count == 0) is a copy."""
    args = _avg_tables_args("avg_update", table_host, table, chunks_host, chunks, count, hyper, guard)
    assert count.dtype == torch.int64 and count.numel() == 1
    for h in (hyper_host, hyper):
        assert h is None or (h.dtype == torch.float32 and h.numel() >= 1 and h.is_contiguous())
    assert hyper_host is None or not hyper_host.is_cuda
    sfhip._call("sf_avg_update", *args, int(mode), _vp(hyper_host), _vp(hyper), _vp(count), _vp(guard),
                tag="avg_update")


def avg_exchange(table_host, table, chunks_host, chunks, op):
    """One `sf_avg_exchange` launch over the table, all three kinds: op 0 swaps average and source element by element,
    op 1 copies average -> source, op 2 source -> average."""
    args = _avg_tables_args("avg_exchange", table_host, table, chunks_host, chunks)
    sfhip._call("sf_avg_exchange", *args, int(op), tag="avg_exchange")


class _PairTable(object):
    """The address table of a list of (average view, source tensor, kind) pairs in host and device memory, cached by
    the source addresses and rebuilt when one moves.  Empty tensors have no row."""

    def __init__(self, who):
        self.who = who
        self.sig = None
        self.table = self.chunks = self.table_dev = self.chunks_dev = None

    def args(self, pairs):
        sig = [s.data_ptr() for _, s, _ in pairs]
        if sig != self.sig:
            entries = []
            for a, s, kind in pairs:
                if not s.is_cuda:
                    raise sfhip.SfhipError("%s: tensor on %s — the averaging kernels run on the GPU only (no CPU "
                                           "fallback)" % (self.who, s.device))
                if s.device != a.device or s.device.index != torch.cuda.current_device():
                    raise sfhip.SfhipError("%s: source on %s, average on %s, current device cuda:%d" % (
                        self.who, s.device, a.device, torch.cuda.current_device()))
                if not s.is_contiguous() or s.dtype != a.dtype or s.numel() != a.numel():
                    raise ValueError("%s: a source must be contiguous and match its average in dtype and size, got %s "
                                     "%s for %s %s" % (self.who, s.dtype, tuple(s.shape), a.dtype, tuple(a.shape)))
                if a.numel() > 0:
                    entries.append((a.data_ptr(), s.data_ptr(), a.numel(), kind))
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("%s under stream capture needs a new address table, which takes host-to-device "
                                   "copies — warm up eagerly first (run the same step outside the capture)" % self.who)
            if not entries:
                self.table = None
            else:
                dev = pairs[0][0].device
                self.table, self.chunks = build_avg_tables(entries, sfhip.lib().sf_sgd_chunk_elems())
                self.table_dev, self.chunks_dev = self.table.to(dev), self.chunks.to(dev)
            self.sig = sig
        if self.table is None:
            return None
        return self.table, self.table_dev, self.chunks, self.chunks_dev


def _check_decay(decay):
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError("HipAveragedModel: decay must be a number in [0, 1] or None, got %r" % (decay,))
    if not 0.0 <= d <= 1.0:  # (a NaN fails both; torch's get_ema_multi_avg_fn refuses the same range)
        raise ValueError("HipAveragedModel: invalid decay value %r — give one in [0, 1]" % (decay,))
    return d


class HipAveragedModel(object):
    """`torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=use_buffers)` for
    a float `decay`, the SWA default (the equal-weight mean) for `decay=None` — without a second module:

        ema = HipAveragedModel(model, decay=0.999)
        loss.backward(); opt.step(guard=loss_fun.guard); ema.update_parameters(guard=loss_fun.guard)
        with ema.applied():
            model.eval(); preds = model(inputs)         # the averaged weights, through the model's own caches

    Storage: ONE float32 allocation holds a 16-byte aligned flat view per parameter and float buffer, one int64
    allocation the integer buffers; `averaged` maps each name of `chain(named_parameters(), named_buffers())`, in that
    order, to its view (shaped as the tensor) and `n_averaged` is an int64 tensor in device memory.  They start as a
    copy of the model, as torch's deep copy does.  float32 parameters only.

    `update_parameters(model=None, guard=None)` is ONE native call (`sf_avg_update`): the first update copies, later
    ones are torch's lerp by 1 - decay (EMA) or by 1 / (n_averaged + 1) (SWA), and the call itself advances
    `n_averaged`.  With `use_buffers=False` the float buffers are copied from the model instead, as torch does.  `guard`
    (a device float: the loss's, clipper's or LARS's) switches the whole update off when raised, the count included.
    The address table is cached by the source addresses and rebuilt when one moves (a re-assigned parameter or buffer
    is seen; a replaced submodule needs a new object); under stream capture a rebuild or a
    first call raises — warm up eagerly first — and after that the call is capturable (no host sync, no allocation).
    The decay lives in device memory: `set_decay(d)` uploads only when the value changed, so a replayed step reads the
    current one; a warm-up schedule such as min(decay, (1 + n) / (10 + n)) is the caller's host arithmetic.

    Integer buffers (`num_batches_tracked`) are always COPIED from the model.  torch's EMA pushes them through float32
    arithmetic (`p_ema * decay + p_model * (1 - decay)`, truncated back to int64) and its SWA through an integer
    addcdiv; this class does not reproduce either — a batch count has no meaningful average.

    `swap()` exchanges averages and model tensors in one launch (`sf_avg_exchange`) and bumps the engine's parameter
    epoch; `applied()` is the context manager around two swaps; `copy_to_model()` / `reset_from_model()` copy one way.
    None of them allocates.  `state_dict()` / `load_state_dict()` use AveragedModel's own keys (`n_averaged`,
    `module.<name>` in the module's state-dict order): a state dict saved from torch's AveragedModel of the same model
    loads here and the reverse."""

    def __init__(self, model, decay=None, use_buffers=True):
        self.model = model
        self.use_buffers = bool(use_buffers)
        self.decay = None if decay is None else _check_decay(decay)
        self.mode = MODE_MEAN if decay is None else MODE_EMA
        named = list(chain(model.named_parameters(), model.named_buffers()))
        n_params = sum(1 for _ in model.parameters())
        if not named:
            raise ValueError("HipAveragedModel: the model has no parameters and no buffers")
        for i, (name, t) in enumerate(named):
            if i < n_params:
                if t.dtype != torch.float32:
                    raise ValueError("HipAveragedModel: parameter of dtype %s — float32 only" % t.dtype)
                if not t.is_contiguous():
                    raise ValueError("HipAveragedModel: parameters must be contiguous")
            elif t.dtype not in (torch.float32, torch.int64) or not t.is_contiguous():
                raise ValueError("HipAveragedModel: buffer %s of dtype %s — contiguous float32 or int64 only" % (
                    name, t.dtype))
        dev = named[0][1].device
        floats = [(n, t) for n, t in named if t.dtype == torch.float32]
        words = [(n, t) for n, t in named if t.dtype == torch.int64]
        self._block, fviews = carve_views([t.numel() for _, t in floats], dev)
        self._words = torch.zeros((sum(t.numel() for _, t in words),), dtype=torch.int64, device=dev)
        views, off = {}, 0
        for (n, t), v in zip(floats, fviews):
            views[n] = v.view_as(t)
        for n, t in words:
            views[n] = self._words[off:off + t.numel()].view_as(t)
            off += t.numel()
        self.averaged = OrderedDict((n, views[n]) for n, _ in named)
        self._kinds = [KIND_WORDS if t.dtype == torch.int64 else
                       (KIND_AVG if i < n_params or self.use_buffers else KIND_COPY) for i, (_, t) in enumerate(named)]
        self.n_averaged = torch.zeros((), dtype=torch.int64, device=dev)
        with torch.no_grad():
            for (n, t) in named:
                self.averaged[n].copy_(t.detach())
        self._owners = []  # per name: the module dict that holds the tensor and its key there (no module walk per step)
        for n, _ in named:
            owner = model.get_submodule(n.rpartition(".")[0])
            key = n.rpartition(".")[2]
            self._owners.append((owner._parameters if key in owner._parameters else owner._buffers, key))
        self._tab = _PairTable("HipAveragedModel")
        self._stage = _HyperStage()
        self._w_host = self._w_dev = None  # 1 - decay as float32: the host value and its copy in device memory
        if self.decay is not None:
            self._w_host = torch.tensor([1.0 - self.decay], dtype=torch.float32)
            if dev.type == "cuda":
                self._w_dev = self._w_host.to(dev)

    # ---- the decay in device memory
    def set_decay(self, decay):
        """A new decay for the updates that follow: one small copy from a pinned staging row on the current stream, and
        only when the float32 weight 1 - decay changed.  Returns whether anything was copied."""
        if self.decay is None:
            raise ValueError("HipAveragedModel.set_decay: made with decay=None (the equal-weight mean has no decay)")
        self.decay = _check_decay(decay)
        w = torch.tensor([1.0 - self.decay], dtype=torch.float32)
        if torch.equal(w, self._w_host):
            return False
        self._w_host = w
        if self._w_dev is None:
            return False  # a CPU model: nothing to upload (update_parameters refuses it)
        self._stage.upload(w, self._w_dev)
        return True

    # ---- the table
    def _pairs(self, model):
        if model is self.model:  # the owning dicts, looked up by name: a re-assigned parameter or buffer is seen
            src = [d[k] for d, k in self._owners]
        else:
            src = list(chain(model.parameters(), model.buffers()))
        if len(src) != len(self.averaged):
            raise ValueError("HipAveragedModel: the model has %d parameters and buffers, the averages %d" % (
                len(src), len(self.averaged)))
        return [(a, s, k) for a, s, k in zip(self.averaged.values(), src, self._kinds)]

    def _args(self, model):
        args = self._tab.args(self._pairs(self.model if model is None else model))
        if args is None:
            raise ValueError("HipAveragedModel: every tensor of the model is empty")
        return args

    @torch.no_grad()
    def update_parameters(self, model=None, guard=None):
        """Average `model` (default: the one given at construction) into the averages: one `sf_avg_update` call."""
        if guard is not None and (not guard.is_cuda or guard.dtype != torch.float32):
            raise ValueError("HipAveragedModel.update_parameters: guard is a float32 tensor on the GPU")
        avg_update(*self._args(model), self.mode, self.n_averaged, hyper_host=self._w_host, hyper=self._w_dev,
                   guard=guard)

    # ---- evaluation on the averaged weights
    def _exchange(self, op):
        avg_exchange(*self._args(None), op)
        engine.parameters_changed()

    @torch.no_grad()
    def swap(self):
        """Exchange the averages and the model's tensors: one launch, then the engine's parameter epoch moves so that
        every packed weight, bf16 plane and folded BN is derived again.  Twice restores every bit."""
        self._exchange(OP_SWAP)

    @contextlib.contextmanager
    def applied(self):
        """`with ema.applied():` — the model holds the averaged weights inside the block and its own behind it."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def copy_to_model(self):
        """averages -> model (the trained weights are overwritten)."""
        self._exchange(OP_TO_SOURCE)

    @torch.no_grad()
    def reset_from_model(self):
        """model -> averages; `n_averaged` is left as it is."""
        avg_exchange(*self._args(None), OP_FROM_SOURCE)

    # ---- checkpoints with AveragedModel's keys
    def _state_names(self):
        return list(self.model.state_dict().keys())

    def state_dict(self):
        out = OrderedDict([("n_averaged", self.n_averaged)])
        for k in self._state_names():
            out["module." + k] = self.averaged[k]
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        want = ["n_averaged"] + ["module." + k for k in self._state_names()]
        for k in want:
            if k not in state_dict:
                raise KeyError("HipAveragedModel.load_state_dict: missing key %r" % k)
        for k in state_dict:
            if k not in want:
                raise KeyError("HipAveragedModel.load_state_dict: unexpected key %r" % k)
        for k in want:
            dst = self.n_averaged if k == "n_averaged" else self.averaged[k[len("module."):]]
            src = state_dict[k]
            if not torch.is_tensor(src) or tuple(src.shape) != tuple(dst.shape):
                raise ValueError("HipAveragedModel.load_state_dict: %r has shape %s, expected %s" % (
                    k, tuple(getattr(src, "shape", ())), tuple(dst.shape)))
        for k in want:
            dst = self.n_averaged if k == "n_averaged" else self.averaged[k[len("module."):]]
            dst.copy_(state_dict[k].detach().to(device=dst.device, dtype=dst.dtype))


def construct_hip_ema(model, cfg):
    """SOLVER.EMA_ON / SOLVER.EMA_DECAY (0.999) / SOLVER.EMA_USE_BUFFERS (True) read with `.get` (config/defaults.py
    mirrors the reference's key set, which has none of them: set them on a config that allows new keys) -> a
    HipAveragedModel over `model`, or None when EMA_ON is missing or false."""
    node = cfg.SOLVER
    if not node.get("EMA_ON", False):
        return None
    return HipAveragedModel(model, decay=float(node.get("EMA_DECAY", 0.999)),
                            use_buffers=bool(node.get("EMA_USE_BUFFERS", True)))
