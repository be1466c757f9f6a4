"""Host-side glue between the nn.Module tree (parameter containers with the reference's names) and the
libsfhip kernels: parameter preprocessing caches (packed weights, folded eval-mode BN), the fused
conv(+BN)(+residual)(+ReLU) unit, the stem trick, and the NCTHW <-> NDHWC boundary handling that lets
every top-level child be called on its own with the reference's list-of-NCTHW-tensors convention
(Grad-CAM contract, wdf_visualization/gradcam_video.py:92-105)."""
import os
import threading
import weakref

import torch
import torch.nn as nn

import sfhip
from sfhip import Act

_tls = threading.local()


class internal(object):
    """Context: children exchange NDHWC `Act`s instead of converting back to NCTHW tensors."""

    def __enter__(self):
        self.prev = getattr(_tls, "depth", 0)
        _tls.depth = self.prev + 1

    def __exit__(self, *a):
        _tls.depth = self.prev


def is_internal():
    return getattr(_tls, "depth", 0) > 0


def enter(xs):
    """list of NCTHW tensors or Acts -> list of Acts."""
    return [x if isinstance(x, Act) else sfhip.from_ncthw(x) for x in xs]


def leave(acts):
    """list of Acts -> what the caller expects (Acts inside a model forward, NCTHW tensors otherwise)."""
    if is_internal():
        return acts
    return [sfhip.to_ncthw(a) for a in acts]


# ------------------------------------------------------------------------------------------------ tape
class Tape(object):
    """Reverse-mode tape of ONE training forward.  Activation gradients live in zero-initialised NDHWC
    buffers shaped like their forward buffers (keyed by address), and every backward op ACCUMULATES into
    them — that is autograd's fan-in sum for residual branches and for the two consumers each pathway tensor
    has in the lateral fusions.  Parameter gradients are collected per nn.Parameter."""

    def __init__(self):
        self.ops = []
        self.gbuf = {}
        self.pgrads = {}
        self.out_act = None
        self.sink = None  # {param: its .grad} when parameter gradients are accumulated in place (set_grad_sink)
        self.side = None  # the side stream ops are being recorded for (run_paths), None = the caller's stream
        self.serial = getattr(_tls, "serial", False)  # the model keeps one stream (collective-carrying layers)
        self.input_ids = {}    # id(clip tensor) -> input index, for the inputs whose gradient autograd asked for
        self.input_grads = {}  # input index -> dL/d(clip), NCTHW (written by the stems' backward)
        self.joins = set()  # companion streams with weight-gradient work in flight (joined at the end of backward)
        self.model = None   # the model whose forward this tape records (milestone hooks are bound to it)
        self.capturing = False  # the backward is being captured into a hipGraph (no companion-stream forks then)
        self.arena = None   # backward of a small model: ONE zero-filled tensor the gradient buffers are cut from
        self.arena_off = 0
        self.zero_floats = -1  # >= 0 while the backward runs: floats of zero-initialised buffers it has asked for
        self.armed = True        # False: ops are not recorded yet (EvalTape before its target boundary)
        self.param_grads = True  # False: weight / bias gradients are neither computed nor collected (EvalTape)

    def pgrad_target(self, param):
        """The tensor kernels may accumulate this parameter's gradient into directly, or None."""
        if self.sink is None:
            return None
        g = self.sink.get(param)
        return g if g is not None and g.is_contiguous() else None

    def grad_of(self, act):
        key = act.buf.data_ptr()
        g = self.gbuf.get(key)
        if g is None:
            n = act.buf.numel()
            nal = (n + 63) // 64 * 64
            if self.zero_floats >= 0:
                self.zero_floats += nal
            if self.arena is not None and self.arena_off + nal <= self.arena.numel() and \
                    self.arena.device == act.buf.device:
                g = self.arena[self.arena_off:self.arena_off + n]
                self.arena_off += nal
            else:
                g = torch.zeros(n, dtype=torch.float32, device=act.buf.device)
            self.gbuf[key] = g
        return Act(g.view(act.buf.shape), act.coff, act.C)

    def has_grad(self, act):
        return act.buf.data_ptr() in self.gbuf

    def grad_dst(self, act, whole=True):
        """(gradient buffer of `act`, accumulate) for a backward op about to issue dL/d(act) — the ONE statement of the
        first-writer rule.  A whole-buffer activation that has no gradient yet (and `whole`: the op writes every
        element of it) gets an UNINITIALISED buffer and accumulate=False: the caller is the first — usually only —
        writer and must overwrite every element, which saves the zero fill and the read of an accumulate.  In every
        other case (a channel slice, a buffer that already holds a fan-in sum, not `whole`) it is grad_of's
        zero-initialised or existing buffer and accumulate=True."""
        key = act.buf.data_ptr()
        if not whole or key in self.gbuf or act.coff != 0 or act.cs != act.C:
            return self.grad_of(act), True
        g = torch.empty(act.buf.numel(), dtype=torch.float32, device=act.buf.device)
        self.gbuf[key] = g
        return Act(g.view(act.buf.shape), 0, act.C), False

    def record(self, fn):
        self.ops.append((fn, self.side))

    def add_pgrad(self, param, g):
        g = g.reshape(param.shape)
        tgt = self.sink.get(param) if self.sink is not None else None
        if tgt is not None:
            tgt.add_(g)
            return
        cur = self.pgrads.get(param)
        self.pgrads[param] = g if cur is None else cur + g

    def add_pgrads(self, params, grads):
        """add_pgrad for several parameters at once: with a gradient sink (FlatGradients) the accumulations are ONE
        multi-tensor launch instead of one small add per parameter (the q | k | v projections of an attention: six adds on
        the path between its weight gradient and its data gradient)."""
        tgts = [self.sink.get(p) if self.sink is not None else None for p in params]
        if all(t is not None for t in tgts) and len(tgts) > 1:
            torch._foreach_add_(tgts, [g.reshape(p.shape) for p, g in zip(params, grads)])
            return
        for p, g in zip(params, grads):
            self.add_pgrad(p, g)

    def _replay(self):
        """The recorded ops in reverse, each on the stream it was recorded for: ops recorded inside run_paths on the
        side stream run there again; the region's join / fork markers become the backward pass's fork / join."""
        for fn, side in reversed(self.ops):
            if side is None:
                fn()
            else:
                with torch.cuda.stream(side):
                    fn()

    def backward(self):
        self._open_arena()
        self.capturing = bool(torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())
        asked = -1
        try:
            self._replay()
            for wg in self.joins:
                _sync_streams(wg, torch.cuda.current_stream(wg.device))
            asked = self.zero_floats
        finally:
            # also after a failed replay (SfhipError, OOM): no arena stays referenced, and no later grad_of outside a
            # backward is counted against — or cut from — a partly used, no longer zero one
            self.joins = set()
            self.ops = []
            self.zero_floats = -1
            self.gbuf = {}
            self.arena = None
            self.arena_off = 0
            self.capturing = False
        if self.model is not None and asked >= 0:   # published only by a backward that ran to its end
            self.model.__dict__["_sf_arena_floats"] = asked

    def _open_arena(self):
        """Launch-bound models (cfg #1: ~115 gradient buffers of a few KB each): the zero-initialised gradient buffers of
        one backward come out of ONE zero-filled tensor — one fill launch instead of one per buffer.  Sized by what the
        previous backward of the same model asked for; made here, on the stream the backward starts on and before any
        side stream is forked, so every later use is ordered behind the fill.  Only models whose buffers total at most
        64 MB (ARENA_MAX_FLOATS) take it: a large model keeps one fill per buffer, which overlaps with the backward's
        kernels instead of delaying its first one (an arena for just the SMALL buffers of a large model was tried: cfg #3
        51.98 against 51.60 ms, two alternations on one box; cfg #5 at 2 clips unchanged)."""
        self.zero_floats = 0
        if self.model is None or self.out_act is None:
            return
        want = self.model.__dict__.get("_sf_arena_floats", 0)
        if 0 < want <= ARENA_MAX_FLOATS:
            self.arena = torch.zeros(want, dtype=torch.float32, device=self.out_act.buf.device)
            self.arena_off = 0


def tape():
    t = getattr(_tls, "tape", None)
    return t if t is None or t.armed else None


class EvalTape(Tape):
    """Tape of ONE eval-mode forward that yields ACTIVATION gradients only (models/gradcam.py; reference
    wdf_visualization/gradcam_video.py:107-157).  Recording starts at the output boundary of the top-level child
    `target` (engine.boundary): everything before it runs as the plain eval forward and leaves no closure, so the
    replay ends at the target.  No weight-gradient kernel is launched, no parameter's .grad is read or written and no
    gradient sink is consulted."""

    def __init__(self, target):
        super(EvalTape, self).__init__()
        self.armed = False
        self.param_grads = False
        self.target = target
        self.target_acts = None  # the target child's outputs (Acts), set when recording starts
        self.out = None          # the head's eval output [N, classes]
        self.dout = None         # dL/d(out), set by backward()

    def pgrad_target(self, param):
        return None

    def add_pgrad(self, param, g):
        pass

    def add_pgrads(self, params, grads):
        pass

    def backward(self, dout):
        """Replay from dL/d(out) = dout [N, classes] down to the target boundary; returns dL/d(target outputs) as
        Acts (views of the gradient buffers, which then belong to the caller)."""
        if self.target_acts is None or self.out is None:
            raise RuntimeError("the eval tape saw no boundary named %r, or no head output" % (self.target,))
        self.dout = dout.contiguous()
        try:
            self._replay()
            return [self.grad_of(a) for a in self.target_acts]
        finally:
            self.ops = []
            self.gbuf = {}
            self.dout = None


class eval_taping(object):
    """Context entered by models/gradcam.py only: the eval forward inside it records an EvalTape from the output of the
    top-level child `target` on.  Nothing outside it changes: a plain eval forward and model.train() steps issue the
    launches they always did."""

    def __init__(self, target):
        self.t = EvalTape(target)

    def __enter__(self):
        self.prev = getattr(_tls, "tape", None)
        _tls.tape = self.t
        return self.t

    def __exit__(self, *a):
        _tls.tape = self.prev


def boundary(name, x):
    """Called by the ResNet-family models' _forward_impl behind each top-level child with its outputs (Acts).  Under an
    EvalTape whose target is `name` this is where recording starts; otherwise nothing happens."""
    t = getattr(_tls, "tape", None)
    if isinstance(t, EvalTape) and not t.armed and name == t.target:
        join_pending(x[0].buf.device)  # a fusion's deferred join: the target's outputs are complete on this stream
        t.target_acts = list(x)
        t.armed = True
    return x


_MILESTONE_HOOKS = weakref.WeakKeyDictionary()  # model -> hook: a hook only ever sees the backward of ITS model


def set_milestone_hook(fn, model):
    """fn(child_name, tape) is called DURING the backward pass of `model` at the point where every gradient of the
    top-level child `child_name` and of all children after it has been issued (on the caller's stream, the side stream
    — joined by then — or a companion stream listed in tape.joins).  utils.distributed.FlatGradients uses it to start
    the all-reduce of the finished tail of the flat gradient buffer while the earlier stages' backward still runs (the
    reference gets the same overlap from DistributedDataParallel's buckets, models/build.py:39-43).  fn = None removes
    the model's hook."""
    if fn is None:
        _MILESTONE_HOOKS.pop(model, None)
    else:
        _MILESTONE_HOOKS[model] = fn


def milestone(name):
    """Called by the models' _forward_impl in front of each top-level child."""
    t = tape()
    if t is None or t.model is None:
        return
    hook = _MILESTONE_HOOKS.get(t.model)
    if hook is not None:
        t.record(lambda: hook(name, t))


# ------------------------------------------------------------------------------------------------ two streams
# The Slow and the Fast pathway are independent between lateral fusions, and so are the two directions of a CMDA
# fusion: the Fast pathway is a string of small-channel, HBM-bound kernels (and tiny grids), the Slow pathway of
# MFMA-bound ones.  run_paths issues the second callable on a side stream so the two overlap on the GPU; forward and
# backward regions are delimited by events (fork: side waits for the caller's stream; join: the caller's stream waits
# for side), which is also all the ordering the caching allocator needs: a block is only ever re-used by the stream
# that allocated it, and every region starts / ends by ordering that stream against the other.
OVERLAP_PATHS = os.environ.get("SF_OVERLAP_PATHS", "1") != "0"
_SIDE = {}


def _side_stream(device):
    s = _SIDE.get(device)
    if s is None:
        # normal priority (also for the companion streams).  High priority for this stream gained 0.25 ms of the eager
        # train step but cost 13-70 % of the eval forward's hipGraph replay (442 -> 383 clips/s, cfg #1 2866 -> 600):
        # graph nodes captured on a high-priority stream replay through a slower path on this stack
        s = _SIDE[device] = torch.cuda.Stream(device=device)
    return s


_COMPANION = {}


def _companion_stream(parent):
    """A stream paired with `parent` (the caller's or the side stream) for work only needed at the end of backward."""
    key = (parent.device, parent.cuda_stream)
    s = _COMPANION.get(key)
    if s is None:
        s = _COMPANION[key] = torch.cuda.Stream(device=parent.device)
    return s


def _sync_streams(first, then):
    ev = torch.cuda.Event()
    ev.record(first)
    then.wait_event(ev)


def run_paths(fns, device, defer_join=False):
    """[f() for f in fns] with fns[1] issued on the side stream (two callables on a CUDA device; otherwise serial).
    defer_join: do not make the caller's stream wait for the side stream at the end of the FORWARD region — only
    valid when the next work on the caller's stream does not read what fns[1] produced before the next region's
    join (a CMDA fusion followed by a stage: the attention keeps running beside the Slow pathway's next stage).
    The next region forks onto the same side stream, so it is ordered behind the deferred work without a join."""
    if not OVERLAP_PATHS or getattr(_tls, "serial", False) or len(fns) != 2 or device.type != "cuda":
        return [f() for f in fns]
    t = tape()
    if t is not None and t.side is not None:
        return [f() for f in fns]  # already inside a region
    main, side = torch.cuda.current_stream(device), _side_stream(device)

    def bwd_join():  # last op of the region's backward
        _sync_streams(side, torch.cuda.current_stream(device))

    def bwd_fork():  # first op of the region's backward
        _sync_streams(torch.cuda.current_stream(device), side)

    if t is not None:
        t.record(bwd_join)
    _sync_streams(main, side)                                                       # forward: fork
    out0 = fns[0]()
    with torch.cuda.stream(side):
        if t is not None:
            t.side = side
        try:
            out1 = fns[1]()
        finally:
            if t is not None:
                t.side = None
    if not defer_join:
        _sync_streams(side, main)                                                   # forward: join
        _tls.pending_side = None  # (a deferred region ran on `side` too: joined here as well)
    else:
        _tls.pending_side = side
    if t is not None:
        t.record(bwd_fork)
    return [out0, out1]


def join_pending(device):
    """Make the caller's stream wait for a region whose forward join was deferred and never followed by another
    region (end of a forward pass)."""
    pend = getattr(_tls, "pending_side", None)
    if pend is not None:
        _sync_streams(pend, torch.cuda.current_stream(device))
        _tls.pending_side = None


class taping(object):
    def __init__(self, t):
        self.t = t

    def __enter__(self):
        self.prev = getattr(_tls, "tape", None)
        _tls.tape = self.t

    def __exit__(self, *a):
        _tls.tape = self.prev


def _colsum(act):
    """per-channel sum over all rows (bias gradients)."""
    mean, _ = sfhip.channel_stats(act)
    return mean * float(act.rows)


def _record_conv(x, conv_weight, conv_bias, wp_shape, gsrc, kernel, stride, padding, dilation, x_needs_grad=True,
                 cin=None, unpack=None, fold_kw=0):
    """Backward of a dense conv whose output gradient will be found in `gsrc` (an Act).  fold_kw: the stem layout
    (packed channel = (kw, ci)); `unpack` maps the packed gradient to the parameter's layout on the autograd path."""
    t = tape()
    if t is None:
        return
    cout = conv_weight.shape[0]

    def wgrad(g):
        tgt = t.pgrad_target(conv_weight)
        if tgt is not None:  # partial sum + un-pack + accumulate into .grad in one kernel
            real_cin = conv_weight.shape[1]
            sfhip.conv_wgrad(x, g, cout, kernel, stride, padding, dilation, cin=cin, cin_pad=wp_shape[2],
                             finish_into=(tgt, real_cin, fold_kw))
        else:
            dwp = sfhip.conv_wgrad(x, g, cout, kernel, stride, padding, dilation, cin=cin, cin_pad=wp_shape[2])
            t.add_pgrad(conv_weight, unpack(dwp) if unpack else sfhip.unpack_conv_weight_grad(dwp, conv_weight.shape))
        if conv_bias is not None:
            t.add_pgrad(conv_bias, _colsum(g))

    def bwd():
        g = gsrc() if callable(gsrc) else gsrc
        dev = x.buf.device
        if not t.param_grads:  # activation gradients only (EvalTape)
            pass
        # The fork costs two cross-stream hand-offs: ~15 us each on the device when launched eagerly
        # (tools/microbench/stream_latency.py) — worth it even for the small layers of cfg #3 (52.9 ms forking every
        # layer, 53.2 forking only those estimated above 30 .. 120 us) — but far more as edges of a captured hipGraph:
        # cfg #1's replay went from 9.65 to 6.03 ms, cfg #5's from 43.3 to 34.9 ms and cfg #3's own from 56.6 to 54.1 ms
        # without them.  So: no companion stream while the backward is being CAPTURED; eagerly, every layer forks.
        elif OVERLAP_PATHS and not t.capturing and not t.serial and x_needs_grad and dev.type == "cuda":
            # the weight gradient only feeds the parameter's .grad: issue it on a companion stream so that it
            # overlaps the data gradient (both are short-grid GEMMs on the res4 / res5 layers); joined by
            # Tape.backward before the gradients are handed back
            cur = torch.cuda.current_stream(dev)
            wg = _companion_stream(cur)
            _sync_streams(cur, wg)
            with torch.cuda.stream(wg):
                wgrad(g)
            g.buf.record_stream(wg)  # e.g. the masked-gradient temporary of a bare ReLU dies with this closure
            x.buf.record_stream(wg)
            t.joins.add(wg)
        else:
            wgrad(g)
        if x_needs_grad:
            if conv_weight.dim() == 5 and tuple(conv_weight.shape[2:]) == tuple(kernel):
                wtp = _packed_pair(conv_weight)[1]
            else:  # nn.Linear weights ([K, C]) and other re-shaped uses
                wtp = _cached_t(conv_weight, "_sf_wtp", _key(conv_weight),
                                lambda: sfhip.pack_conv_weight(conv_weight.detach().reshape(
                                    conv_weight.shape[0], conv_weight.shape[1], *kernel).transpose(0, 1).contiguous()))
            dx, acc = t.grad_dst(x)  # first consumer of x: write, do not accumulate
            sfhip.conv_dgrad(g, wtp, x, kernel, stride, padding, dilation, out=dx, accumulate=acc)

    t.record(bwd)


_PCACHE = {}


# Parameter-derived tensors (packed weights, their planes, folded BN ...) that a hipGraph capture has read or written.
# They are allocated EAGERLY (outside the graph's private pool) and live in per-parameter caches; an eager forward after
# the capture that finds them stale (an eval pass between replays) replaces the cache entry, and without this table
# the old tensors would go back to the allocator while the graph still reads and re-packs into them on every replay.
_CAPTURE_KEEP = {}


def _keep_if_capturing(obj):
    if getattr(_tls, "capturing", False):
        _CAPTURE_KEEP[id(obj)] = obj
    return obj


def _cached_t(tensor, slot, key, make):
    """cache keyed on a tensor (parameters are not nn.Modules).  The entry lives ON the tensor object, so it dies
    with it: a global table keyed by id() would hand a new parameter that re-uses a freed one's id, address and
    version the old one's packed weights."""
    store = tensor.__dict__.setdefault("_sf_cache", {})
    c = store.get(slot)
    if c is None or c[0] != key:
        with torch.no_grad():
            c = (key, make())
        store[slot] = c
    return _keep_if_capturing(c[1])


# Everything derived from parameters (packed conv weights and their bf16 planes, folded BN affines, q/k/v stacks, ...)
# is cached per (address, torch version counter) of its sources.  torch's FUSED optimizers (torch.optim.SGD / Adam
# with fused=True: one multi-tensor kernel, torch._fused_sgd_) update the parameters WITHOUT moving their version
# counters, so the counter alone would leave every cache on the pre-update weights — silently: the step still runs,
# on frozen packed weights (found by tests/test_graph_train_gpu.py in round 5: the replayed graph, whose re-pack is a
# captured launch, disagreed with eager steps that skipped it).  Every optimizer step of the process therefore bumps
# an epoch that is part of every cache key (a global post-step hook: fires for any torch.optim.Optimizer, fused or
# not); code that writes parameters through raw pointers calls parameters_changed() itself.
_PARAM_EPOCH = 0


def parameters_changed(*_unused):
    """Invalidate every parameter-derived cache of the HIP path (packed weights, folded BN, ...)."""
    global _PARAM_EPOCH
    _PARAM_EPOCH += 1


def replay(graph):
    """graph.replay() for a hipGraph that holds a TRAINING step (forward, backward, optimizer update) — the form every
    caller of such a graph must use.  A replayed optimizer kernel moves the parameters without running torch's Python
    optimizer hooks and without touching version counters, and the re-pack launches captured in the graph refresh the
    copies in the GRAPH's memory pool, not the ones eager code reads: without the epoch bump an eager forward after the
    replays (an eval pass, a checkpoint's BN fold) would silently reuse packed weights, bf16 planes, folded BN and q/k/v
    stacks from before them (tests/test_graph_train_gpu.py::test_eval_after_replays_sees_the_trained_weights)."""
    graph.replay()
    parameters_changed()


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook
    _STEP_HOOK = _register_step_hook(lambda optimizer, args, kwargs: parameters_changed())
except ImportError:  # pragma: no cover — torch without global optimizer hooks
    _STEP_HOOK = None


def _key(*tensors):
    return (_PARAM_EPOCH,) + tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


def _cached(mod, slot, key, make):
    c = mod.__dict__.get(slot)
    if c is None or c[0] != key:
        with torch.no_grad():
            c = (key, make())
        mod.__dict__[slot] = c
    return _keep_if_capturing(c[1])


def check_bn(bn):
    from .batchnorm_helper import SubBatchNorm3d
    if not isinstance(bn, (nn.BatchNorm3d, SubBatchNorm3d)):
        raise NotImplementedError("unsupported normalisation layer on the HIP path: %s" % type(bn))


def _sub_bn(bn):
    from .batchnorm_helper import SubBatchNorm3d
    return isinstance(bn, SubBatchNorm3d)


def _sync_bn(bn):
    from .batchnorm_helper import NaiveSyncBatchNorm3d
    from slowfast.utils import distributed as du
    return isinstance(bn, NaiveSyncBatchNorm3d) and du.get_local_size() > 1


_NBT = None  # inside run_model: the num_batches_tracked buffers to bump with ONE foreach add at the end


def _bump(counter):
    if _NBT is not None:
        _NBT.append(counter)
    else:
        counter.add_(1)


def _plain_bn(bn):
    return not _sub_bn(bn) and not _sync_bn(bn)


def _bn_train_stats(bn, z, conv_stats=None):
    """(mean, invstd, scale, shift, nsplit, gamma_for_backward, sync_hook) of a training-mode norm layer; updates
    the running statistics in place exactly as the reference layer would.  conv_stats: per-tile statistics the
    producing conv's epilogue left (sfhip.conv(..., stats=True)) — plain BatchNorm3d then merges those instead of
    reading z again."""
    if _sub_bn(bn):
        S, sb = bn.num_splits, bn.split_bn
        if z.N % S != 0:
            raise ValueError("SubBatchNorm3d: batch %d is not divisible by num_splits %d" % (z.N, S))
        dev = z.buf.device
        w = bn.weight.detach().repeat(S) if bn.affine else torch.ones(S * z.C, device=dev)
        b = bn.bias.detach().repeat(S) if bn.affine else torch.zeros(S * z.C, device=dev)
        track = sb.track_running_stats and sb.running_mean is not None
        m = sb.momentum if sb.momentum is not None else 1.0 / float(int(sb.num_batches_tracked) + 1)
        mean, invstd, scale, shift = sfhip.bn_train_stats(
            z, w, b, sb.eps, m, sb.running_mean if track else None, sb.running_var if track else None, nsplit=S)
        if track:
            _bump(sb.num_batches_tracked)
        return mean, invstd, scale, shift, S, w, None
    track = bn.track_running_stats and bn.running_mean is not None
    m = bn.momentum if bn.momentum is not None else 1.0 / float(int(bn.num_batches_tracked) + 1)
    if _sync_bn(bn):
        from .batchnorm_helper import group_gather_sum
        nd, ng = bn.num_sync_devices, bn.num_groups
        lmean, lvar = sfhip.channel_stats(z)
        lm = lmean.double()
        vec = group_gather_sum(torch.cat([lm, lvar.double() + lm * lm]), nd, ng) / nd  # (mean, E[x^2]) in fp64
        mean64, meansqr = vec[:z.C], vec[z.C:]
        var64 = (meansqr - mean64 * mean64).clamp_min(0.0)
        mean, var = mean64.float(), var64.float()
        invstd = torch.rsqrt(var64 + bn.eps).float()
        scale = (bn.weight.detach() * invstd).contiguous()
        shift = (bn.bias.detach() - mean * scale).contiguous()
        if track:  # the reference keeps the BIASED variance here (batchnorm_helper.py:207-208)
            bn.running_mean += m * (mean - bn.running_mean)
            bn.running_var += m * (var - bn.running_var)
            bn.__dict__.pop("_sf_affine", None)

        def sync(dbeta, dgamma):  # GroupGather.backward: the same gather-and-sum, then the 1/num_sync factor
            tot = group_gather_sum(torch.cat([dbeta, dgamma]).double(), nd, ng) / nd
            return tot[:dbeta.numel()].float().contiguous(), tot[dbeta.numel():].float().contiguous()

        return mean, invstd, scale, shift, 1, bn.weight, sync
    if conv_stats is not None:
        mean, invstd, scale, shift = sfhip.bn_train_stats_merge(
            conv_stats, z.C, bn.weight, bn.bias, bn.eps, m, bn.running_mean if track else None,
            bn.running_var if track else None)
    else:
        mean, invstd, scale, shift = sfhip.bn_train_stats(
            z, bn.weight, bn.bias, bn.eps, m, bn.running_mean if track else None, bn.running_var if track else None)
    if track:  # the kernel wrote the running buffers in place: drop the folded eval-mode affine cache
        bn.__dict__.pop("_sf_affine", None)
        _bump(bn.num_batches_tracked)
    return mean, invstd, scale, shift, 1, bn.weight, None


def _bn_epilogue(bn, z, scale, shift, make_backward, res, relu, rep, out, out_reserve, keep, out_cmul, nsplit=1,
                 eager_sums=False, always_sums=False):
    """The normalise(+residual)(+ReLU)(+T-repeat) pass of an un-fused norm layer on the raw tensor z, and its tape
    closure — what bn_train_apply and bn_frozen_apply share.  keep: only the first `keep` channels are normalised
    (GhostModule [:oup]); out_cmul: the channel-interleaved store (ShuffleNetV2).
    make_backward() is called once, behind the forward pass of a TAPED layer, and returns
    backward(dy, y, zz, dres, dres_accumulate, sink, sums, mask): the layer's one sfhip.*_bwd call, which leaves dL/dz
    in zz (z's own buffer, where the producer's backward looks for it).  dgamma / dbeta go into sink = (weight.grad,
    bias.grad) under the gradient sink, else into sums = two zero-filled [z.C] tensors that are then handed to the
    tape; both are None when the layer owes no parameter gradient.  eager_sums: `sums` is made here, in the forward,
    instead of in the closure; always_sums: the sums are taken even when no parameter receives them."""
    zz = z if keep is None else z.slice(0, keep)
    if keep is not None:
        assert nsplit == 1, "channel-sliced BN (GhostModule) is only defined for plain BatchNorm3d"
        scale, shift = scale[:keep], shift[:keep]
    t = tape()
    shuffled = t is not None and out_cmul != 1
    # taped ReLU / ReLU6 layers: the normalise pass also leaves a byte per 4 channels for the backward's mask, which
    # then reads that instead of the activation (1/16 of the bytes, twice per backward)
    mk = {} if (t is not None and relu) else None
    # taped: a channel-shuffled store is an explicit (taped) strided copy of the dense result
    dst = {} if shuffled else dict(out=out, out_reserve=out_reserve, out_cmul=out_cmul)
    y = sfhip.affine(zz, scale.contiguous(), shift.contiguous(), res=res, relu=relu, rep=rep, nsplit=nsplit, mask=mk,
                     **dst)
    if t is not None:
        mask = mk.get("bytes") if mk else None
        weight, bias = getattr(bn, "weight", None), getattr(bn, "bias", None)
        affine = weight is not None and bias is not None
        backward = make_backward()

        def zeros():
            return torch.zeros(z.C, dtype=torch.float32, device=z.buf.device)

        made = (zeros(), zeros()) if eager_sums else None

        def bwd():
            dres, acc = None, True
            if res is not None:  # first writer of the residual branch's gradient: write it, no zero fill / read
                dres, acc = t.grad_dst(res, whole=nsplit == 1 and res.C == zz.C and rep == 1)
            sink = sums = None
            if always_sums or (affine and t.param_grads):
                wt, bt = (t.pgrad_target(weight), t.pgrad_target(bias)) if (affine and nsplit == 1) else (None, None)
                if wt is not None and bt is not None:  # dgamma / dbeta accumulate into .grad inside the reduction
                    sink = (wt, bt)
                else:
                    sums = made or (zeros(), zeros())
            backward(t.grad_of(y), y, zz, dres, acc, sink, sums, mask)
            if keep is not None and keep < z.C:  # sliced-away channels (GhostModule [:oup]) get no gradient
                rest = z.slice(keep, z.C - keep)
                sfhip.axpy(rest, rest, alpha=0.0, accumulate=False)
            if sums is not None and affine:
                t.add_pgrad(weight, sums[0])
                t.add_pgrad(bias, sums[1])

        t.record(bwd)  # afterwards z's buffer holds dL/dz for the producer's backward
    if shuffled:  # recorded AFTER the BN op so that its backward (the gather) runs first
        return copy_channels(y, out, out_cmul=out_cmul)
    return y


def bn_train_apply(bn, z, res=None, relu=False, rep=1, out=None, out_reserve=(0, 0), keep=None, out_cmul=1,
                   conv_stats=None):
    """Training-mode BatchNorm3d on the raw tensor z: batch statistics (sf_channel_stats), running-stat update
    (momentum, unbiased variance — torch semantics), then ONE normalise(+residual)(+ReLU)(+T-repeat) pass."""
    check_bn(bn)
    with torch.no_grad():
        mean, invstd, scale, shift, nsplit, gamma_b, sync = _bn_train_stats(bn, z, conv_stats)
    sel = slice(None) if nsplit > 1 else slice(0, z.C if keep is None else keep)

    def backward(dy, y, zz, dres, dres_accumulate, sink, sums, mask):
        sfhip.bn_bwd(dy, y, zz, mean[sel], invstd[sel], gamma_b[sel], relu, rep=rep, dres=dres, dz_out=zz,
                     dgamma_out=sums, nsplit=nsplit, sync=sync, grad_sink=sink, mask=mask,
                     dres_overwrite=not dres_accumulate)

    # without the gradient sink the dgamma / dbeta temporaries are made in the forward; with it, only by a layer whose
    # parameters turn out to have no .grad to accumulate into
    return _bn_epilogue(bn, z, scale, shift, lambda: backward, res, relu, rep, out, out_reserve, keep, out_cmul,
                        nsplit=nsplit, eager_sums=not _GRAD_SINK, always_sums=True)


def bn_affine(bn, conv_bias=None):
    """Eval-mode BatchNorm3d as per-channel (scale, bias); a preceding conv bias is folded in."""
    check_bn(bn)
    stat = bn.bn if _sub_bn(bn) else bn  # SubBatchNorm3d evaluates with the aggregated `bn` statistics
    w = getattr(bn, "weight", None)
    b = getattr(bn, "bias", None)

    def make():
        inv = 1.0 / torch.sqrt(stat.running_var + stat.eps)
        scale = w * inv if w is not None else inv
        bias = -stat.running_mean * scale
        if b is not None:
            bias = bias + b
        if conv_bias is not None:
            bias = bias + scale * conv_bias
        return scale.detach().contiguous(), bias.detach().contiguous()

    return _cached(bn, "_sf_affine", _key(w, b, stat.running_mean, stat.running_var, conv_bias), make)


def _taped_training():
    t = tape()
    return t is not None and not isinstance(t, EvalTape)


def bn_unfused(bn):
    """The norm layer runs as its own pass behind a raw producer: in training mode (batch statistics), and in eval mode
    under a TRAINING tape — a frozen BN (utils.misc.frozen_bn_stats, misc.py:246-254), whose gamma / beta still train.
    A plain eval forward and an EvalTape keep the folded one-launch forms."""
    return bn.training or _taped_training()


def bn_apply(bn, z, conv_stats=None, **kw):
    """bn_train_apply or bn_frozen_apply, by bn.training (the decision is per layer)."""
    if bn.training:
        return bn_train_apply(bn, z, conv_stats=conv_stats, **kw)
    return bn_frozen_apply(bn, z, **kw)


def _bn_frozen_stats(bn):
    """(running mean, 1 / sqrt(running var + eps)) of an eval-mode norm layer, cached like bn_affine's pair."""
    stat = bn.bn if _sub_bn(bn) else bn  # SubBatchNorm3d evaluates with the aggregated `bn` statistics
    return _cached(bn, "_sf_frozen", _key(stat.running_mean, stat.running_var),
                   lambda: (stat.running_mean.detach().float().contiguous(),
                            (1.0 / torch.sqrt(stat.running_var + stat.eps)).detach().contiguous()))


def bn_frozen_apply(bn, z, res=None, relu=False, rep=1, out=None, out_reserve=(0, 0), keep=None, out_cmul=1):
    """Eval-mode (frozen) BatchNorm3d on the raw tensor z under a training tape: ONE affine(+residual)(+ReLU)(+T-repeat)
    pass with bn_affine's scale and bias — the running statistics, which are not touched — leaving the byte mask for the
    backward; the tape closure is ONE sf_bn_frozen_bwd pass that writes dL/dz over z (where the producer's backward
    looks for it, as bn_train_apply), the residual's gradient, and accumulates dgamma / dbeta (gamma and beta stay
    trainable: eval() does not freeze them).  Untaped it is the same affine pass and nothing else."""
    check_bn(bn)
    scale, shift = bn_affine(bn)

    def make_backward():
        mean, invstd = _bn_frozen_stats(bn)
        weight = getattr(bn, "weight", None)

        def backward(dy, y, zz, dres, dres_accumulate, sink, sums, mask):
            sfhip.bn_frozen_bwd(dy, y, zz, mean, invstd, weight, relu, rep=rep, dres=dres,
                                dres_overwrite=not dres_accumulate, dz_out=zz,
                                grads=sink if sink is not None else sums, mask=mask)

        return backward

    return _bn_epilogue(bn, z, scale, shift, make_backward, res, relu, rep, out, out_reserve, keep, out_cmul)


def norm_forward(bn, x):
    """A norm layer called on its own (NCTHW tensor or Act): the HIP statistics / normalise kernels."""
    (a,) = enter([x])
    if bn.training:
        y = bn_train_apply(bn, a)
    elif _taped_training():
        y = bn_frozen_apply(bn, a)
    else:
        y = sfhip.affine(a, *bn_affine(bn))
    return leave([y])[0]


ARENA_MAX_FLOATS = 64 << 18  # 64 MB: the largest gradient arena Tape._open_arena makes
_GROUPS_OF = {}  # id(weight) -> groups, for the grouped convs (1 < groups < channels) packed by _group_pairs
_PAIR_WEIGHTS = {}  # id(weight) -> weakref of the dense conv weights that have been packed as a pair (tensors compare
# elementwise, so no WeakSet): repack_all's candidates


def _packed_pair(weight):
    """(forward, data-gradient) packed copies of a dense conv weight, built together by one kernel and cached per
    parameter version (training re-packs every conv once per optimizer step — repack_all does that in one launch)."""
    if not weight.is_cuda:  # CPU construction / state_dict work: torch fallback for the forward layout only
        return sfhip.pack_conv_weight(weight), None
    if id(weight) not in _PAIR_WEIGHTS:
        wid = id(weight)
        _PAIR_WEIGHTS[wid] = weakref.ref(weight, lambda _r, wid=wid: _PAIR_WEIGHTS.pop(wid, None))
    return _cached_t(weight, "_sf_wpair", _key(weight), lambda: sfhip.pack_conv_weight_pair(weight))


def repack_all(model):
    """Re-pack, in ONE launch, every dense, depthwise and grouped conv weight of `model` whose packed pair is stale
    (after an optimizer step: all of them — ~108 launches of ~6 us and 216 allocations otherwise; a grouped conv alone
    was G launches and two allocations).  The packed tensors are overwritten in place:
    the previous step's kernels that read them were joined before the optimizer ran."""
    cand = model.__dict__.get("_sf_pair_params")
    if cand is None or cand[0] != len(_PAIR_WEIGHTS):
        cand = (len(_PAIR_WEIGHTS), [p for p in model.parameters()
                                     if id(p) in _PAIR_WEIGHTS and _PAIR_WEIGHTS[id(p)]() is p])
        model.__dict__["_sf_pair_params"] = cand
    stale, old, slots = [], [], []
    for w in cand[1]:
        store = w.__dict__.get("_sf_cache", {})
        c = store.get("_sf_wpair")
        if c is not None and c[0] != _key(w) and w.is_cuda and w.is_contiguous():
            stale.append(w.detach())
            old.append(c[1])
            slots.append((w, "_sf_wpair", None))
        c = store.get("_sf_wgroups")
        G = _GROUPS_OF.get(id(w))
        if c is not None and G and c[0] != _key(w) and w.is_cuda and w.is_contiguous():
            # a grouped conv's pair = its G per-group packs one after the other: G more records of the same launch,
            # written into the slices of the two tensors the previous version lives in (no allocation)
            wd, (wp, wtp) = w.detach(), c[1]
            cout_g, cin_g = wd.shape[0] // G, wd.shape[1]
            for g in range(G):
                stale.append(wd[g * cout_g:(g + 1) * cout_g])
                old.append((wp[g * cout_g:(g + 1) * cout_g], wtp[g * cin_g:(g + 1) * cin_g]))
                slots.append((w, "_sf_wgroups", (wp, wtp)) if g == 0 else None)
    if len(stale) < 2:
        return
    with torch.no_grad():
        new = sfhip.pack_conv_weight_pairs(stale, old)
    for sl, o, prev in zip(slots, new, old):
        if sl is None:
            continue
        w, name, whole = sl
        if whole is not None and (o[0].data_ptr() != prev[0].data_ptr() or o[1].data_ptr() != prev[1].data_ptr()):
            continue  # a slice was re-allocated (foreign device / dtype): leave the entry stale, _group_pairs re-packs
        w.__dict__["_sf_cache"][name] = (_key(w), _keep_if_capturing(o if whole is None else whole))


def packed_weight(conv):
    if conv.groups == 1:
        return _packed_pair(conv.weight)[0]
    if conv.groups == conv.in_channels and conv.out_channels == conv.in_channels:
        if conv.weight.is_cuda:
            # [taps][pad16(C)]: the transposed half of the pair pack of the [C, 1, kT, kH, kW] parameter — depthwise
            # weights are then re-packed after an optimizer step by repack_all's ONE launch, with the dense ones
            return _packed_pair(conv.weight)[1][0]
        return _cached(conv, "_sf_wp", _key(conv.weight), lambda: sfhip.pack_dw_weight(conv.weight))
    return _group_pairs(conv)


def _group_pairs(conv):
    """(forward, data-gradient) packed weights of a grouped conv (1 < groups < channels) for the one-launch grouped
    kernels, cached per parameter version: wp [Cout][taps][pad(Cin/G)], wtp [Cin][taps][pad(Cout/G)] — group g owns
    output channels [g*Cout/G, (g+1)*Cout/G) and reads input channels [g*Cin/G, (g+1)*Cin/G): nn.Conv3d(groups=G),
    shufflenet_helper.py:48-63 / resnet_helper.py:196-205."""
    w, G = conv.weight, conv.groups
    if conv.in_channels % G or conv.out_channels % G:
        raise ValueError("grouped conv: %d -> %d channels are not divisible by %d groups" % (
            conv.in_channels, conv.out_channels, G))
    if w.is_cuda and id(w) not in _PAIR_WEIGHTS:  # repack_all's candidate list (it re-packs the groups in its one launch)
        wid = id(w)
        _PAIR_WEIGHTS[wid] = weakref.ref(w, lambda _r, wid=wid: (_PAIR_WEIGHTS.pop(wid, None), _GROUPS_OF.pop(wid, None)))
        _GROUPS_OF[wid] = G
    return _cached_t(w, "_sf_wgroups", _key(w), lambda: sfhip.pack_grouped_weight_pair(w, G))


def grouped_conv(x, conv, scale=None, bias=None, relu=False, res=None, out=None, out_reserve=(0, 0), shuffle=False):
    """nn.Conv3d with 1 < groups < channels as a block-diagonal GEMM in ONE launch (sfhip.conv_grouped: the group is
    the grid's z index; input window g -> output window g of the same NDHWC buffers, no tensor is split or
    concatenated).  shuffle: the output is stored channel-shuffled — group g's channel j lands at j*G + g,
    channel_shuffle(., G) of shufflenet_helper.py:22-29 as index math of the stores (eval mode; the taped path shuffles
    after the BN)."""
    k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
    assert x.C == conv.in_channels, (x, conv)
    return sfhip.conv_grouped(x, _group_pairs(conv)[0], conv.groups, k, s, p, d,
                              scale=None if scale is None else scale.contiguous(),
                              bias=None if bias is None else bias.contiguous(), relu=relu, res=res, out=out,
                              shuffle=shuffle, out_reserve=out_reserve)


def _record_grouped_conv(x, conv, gsrc):
    """Backward of grouped_conv (un-shuffled output): ONE weight-gradient launch (+ its finish, straight into the
    parameter's gradient in nn.Conv3d's grouped layout [Cout][Cin/G][k]) and ONE data-gradient launch for all groups."""
    t = tape()
    if t is None:
        return
    G = conv.groups
    k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation

    def bwd():
        g_all = gsrc() if callable(gsrc) else gsrc
        wp, wtp = _group_pairs(conv)
        tgt = t.pgrad_target(conv.weight)
        if not t.param_grads:  # activation gradients only (EvalTape)
            pass
        elif tgt is not None:
            sfhip.conv_wgrad_grouped(x, g_all, G, k, s, p, d, cin_pad=wp.shape[2], finish_into=tgt)
        else:
            dwp = sfhip.conv_wgrad_grouped(x, g_all, G, k, s, p, d, cin_pad=wp.shape[2])
            t.add_pgrad(conv.weight, sfhip.unpack_conv_weight_grad(dwp, tuple(conv.weight.shape)))
        sfhip.conv_dgrad_grouped(g_all, wtp, G, x, k, s, p, d, out=t.grad_of(x), accumulate=True)
        if conv.bias is not None and t.param_grads:
            t.add_pgrad(conv.bias, _colsum(g_all))

    t.record(bwd)


def channel_shuffle(x, groups, out=None, out_reserve=(0, 0)):
    """channel_shuffle(x, G) (shufflenet_helper.py:22-29): channel g*C/G + j -> j*G + g, one launch (taped: the inverse
    permutation — the same kernel with C/G groups — accumulates the gradient in the backward).  The eval path never
    calls it: grouped_conv(shuffle=True) stores so."""
    if groups == 1:
        return x
    if out is None:
        out = sfhip.new_act(x, x.N, x.T, x.H, x.W, x.C, out_reserve[0], out_reserve[1])
    sfhip.channel_shuffle(x, out, groups)
    t = tape()
    if t is not None:
        t.record(lambda: sfhip.channel_shuffle(t.grad_of(out), t.grad_of(x), x.C // groups, accumulate=True))
    return out


def _is_grouped(conv):
    return 1 < conv.groups and not (conv.groups == conv.in_channels and conv.out_channels == conv.in_channels)


def conv_bn_act(x, conv, bn=None, relu=False, res=None, out=None, out_reserve=(0, 0), out_cmul=1, cout=None,
                shuffle=False):
    """nn.Conv3d [+ BatchNorm3d] [+ residual] [+ ReLU].  Eval: ONE kernel launch (BN folded into the
    epilogue).  Training: raw conv -> batch statistics -> one normalise/residual/ReLU pass.  A frozen BN (eval mode
    under a training tape): raw conv -> bn_frozen_apply, the conv's own gradients recorded as in training.
    shuffle (grouped convs only): channel_shuffle(., conv.groups) applied to the result."""
    if _is_grouped(conv):
        assert out_cmul == 1 and cout is None, "grouped convs have their own shuffle"
        if bn is not None and bn_unfused(bn):  # training mode, or frozen (eval mode) under a training tape
            z = grouped_conv(x, conv, bias=conv.bias)
            _record_grouped_conv(x, conv, z)
            if not shuffle:
                return bn_apply(bn, z, res=res, relu=relu, out=out, out_reserve=out_reserve)
            y = bn_apply(bn, z, res=res, relu=relu)
            return channel_shuffle(y, conv.groups, out=out, out_reserve=out_reserve)
        scale, bias = bn_affine(bn, conv.bias) if bn is not None else (None, conv.bias)
        t = tape()
        if t is not None and not isinstance(t, EvalTape):  # (bn is None here: no model has such a layer)
            raise NotImplementedError("taped grouped conv without a norm layer behind it")
        y = grouped_conv(x, conv, scale=scale, bias=bias, relu=relu, res=res, out=out, out_reserve=out_reserve,
                         shuffle=shuffle)
        if t is not None:
            _record_eval_grouped_conv(t, x, conv, y, scale, relu, res, shuffle)
        return y
    assert not shuffle or conv.groups == 1, "channel_shuffle of a depthwise conv's output is not used by any model"
    wp = packed_weight(conv)
    if bn is not None and bn_unfused(bn):  # training mode, or frozen (eval mode) under a training tape
        k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
        st = None
        if conv.groups == 1:
            # plain BatchNorm3d: its batch statistics come out of the conv's epilogue (no extra pass over z)
            want = bn.training and _plain_bn(bn) and bn.affine
            z = sfhip.conv(x, wp, k, s, p, d, bias=conv.bias, stats=want)
            z, st = z if want else (z, None)
            _record_conv(x, conv.weight, conv.bias, wp.shape, z, k, s, p, d)
        else:
            ones = _cached(conv, "_sf_ones", (conv.out_channels, str(x.buf.device)),
                           lambda: torch.ones(conv.out_channels, dtype=torch.float32, device=x.buf.device))
            z = sfhip.dwconv(x, wp, k, s, p, scale=ones if conv.bias is not None else None, bias=conv.bias)
            t = tape()
            if t is not None:
                def bwd_dw():  # z's buffer holds dL/dz after the BN backward
                    tgt = t.pgrad_target(conv.weight)
                    wpk = packed_weight(conv)   # (this step's pack: the forward's may have been re-packed in place)
                    if tgt is not None:  # the reduction's final step accumulates into the parameter's gradient
                        sfhip.dwconv_bwd(x, z, wpk, k, s, p, dx=t.grad_of(x), into=tgt)
                    else:
                        dw = sfhip.dwconv_bwd(x, z, wpk, k, s, p, dx=t.grad_of(x))
                        t.add_pgrad(conv.weight, dw[:, :x.C].t().contiguous())
                    if conv.bias is not None:
                        t.add_pgrad(conv.bias, _colsum(z))

                t.record(bwd_dw)
        return bn_apply(bn, z, res=res, relu=relu, out=out, out_reserve=out_reserve, keep=cout, out_cmul=out_cmul,
                        conv_stats=st)
    if bn is not None:
        scale, bias = bn_affine(bn, conv.bias)
    else:
        scale, bias = None, conv.bias
    k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
    if conv.groups == 1:
        y = sfhip.conv(x, wp, k, s, p, d, scale=scale, bias=bias, relu=relu, res=res, out=out,
                       out_reserve=out_reserve, out_cmul=out_cmul)
        t = tape()
        if isinstance(t, EvalTape):
            _record_eval_conv(t, x, conv, wp, y, scale, relu, res, out_cmul)
        elif t is not None:
            if (res is not None and relu) or out_cmul != 1:  # (bn is None here: a frozen BN took the un-fused branch)
                raise NotImplementedError("taped conv without a norm layer but with a residual behind an activation "
                                          "or an interleaved store")
            if res is not None:  # y = conv(x) + res (NonLocalBlock without its BN): dL/dres += dL/dy
                def bwd_res():
                    sfhip.axpy(t.grad_of(y), t.grad_of(res), 1.0, accumulate=True)
                t.record(bwd_res)
            if relu:  # bare conv + ReLU (no BN): dL/dz = dL/dy masked by the activation's output
                def masked():
                    dz = sfhip.new_act(y, y.N, y.T, y.H, y.W, y.C)
                    return sfhip.act_bwd(t.grad_of(y), y, relu, dz, accumulate=False)
                _record_conv(x, conv.weight, conv.bias, wp.shape, masked, k, s, p, d)
            else:
                _record_conv(x, conv.weight, conv.bias, wp.shape, lambda: t.grad_of(y), k, s, p, d)
        return y
    assert d == (1, 1, 1)
    if scale is None and bias is not None:
        scale = torch.ones_like(bias)
    y = sfhip.dwconv(x, wp, k, s, p, scale=scale, bias=bias, relu=relu, res=res, out=out, cout=cout,
                     out_cmul=out_cmul)
    t = tape()
    if isinstance(t, EvalTape):
        if res is not None or out_cmul != 1 or (cout is not None and cout != x.C):
            raise NotImplementedError("eval-mode tape: a depthwise conv with a residual, a channel-sliced or an "
                                      "interleaved store has no backward here")

        def bwd_dw_eval():  # epilogue backward and data gradient in ONE launch: no dL/dz tensor
            dx, acc = t.grad_dst(x)  # first writer of x's gradient: write, no zero fill / read
            sfhip.dwconv_dgrad_epi(x, t.grad_of(y), y, packed_weight(conv), k, s, p, dx, scale=scale, relu=relu,
                                   accumulate=acc)

        t.record(bwd_dw_eval)
    return y


def _eval_dz_of_y(t, y, scale, relu, res, groups=None):
    """dz_of_y() for the eval-tape conv recorders: the backward of the folded epilogue y = act(scale * z + bias + res)
    into a fresh dL/dz, the residual's gradient in the same pass.  groups None: a dense conv (sf_epilogue_bwd, and
    sf_epilogue_bwd_act only for ReLU6); a number: a grouped conv, always sf_epilogue_bwd_act — with groups > 1 it also
    undoes the channel-shuffled store, so dL/dz is in the conv's own channel order."""
    act = relu if (groups is not None or relu == 6) else None

    def dz_of_y():
        dres, acc = None, True
        if res is not None:  # first writer of the residual branch's gradient: write it, no zero fill / read
            dres, acc = t.grad_dst(res)
        dz = sfhip.new_act(y, y.N, y.T, y.H, y.W, y.C)
        return sfhip.epilogue_bwd(t.grad_of(y), y, dz, scale=scale, relu=relu, act=act, groups=groups or 1, dres=dres,
                                  dres_accumulate=acc)

    return dz_of_y


def _record_eval_grouped_conv(t, x, conv, y, scale, relu, res, shuffle):
    """_record_eval_conv for a grouped conv (1 < groups < channels): the epilogue's backward, then the grouped data
    gradient of the training tape.  No weight or bias gradient."""
    bare = scale is None and res is None and not relu and not shuffle  # conv (+ bias): dL/dz is dL/dy
    _record_grouped_conv(x, conv, (lambda: t.grad_of(y)) if bare else
                         _eval_dz_of_y(t, y, scale, relu, res, groups=conv.groups if shuffle else 1))


def _record_eval_conv(t, x, conv, wp, y, scale, relu, res, out_cmul):
    """Backward of the ONE-launch eval conv y = act(scale * conv(x) + bias + res) on an EvalTape: the epilogue's
    backward (mask from y, the folded BN's scale, the residual's gradient in the same pass), then the data-gradient
    launch of the training tape.  No weight or bias gradient."""
    if out_cmul != 1 or relu not in (False, True, 6):
        raise NotImplementedError("eval-mode tape: an interleaved (out_cmul) store has no backward here")
    bare = scale is None and res is None and not relu  # conv (+ bias): dL/dz is dL/dy
    _record_conv(x, conv.weight, conv.bias, wp.shape,
                 (lambda: t.grad_of(y)) if bare else _eval_dz_of_y(t, y, scale, relu, res),
                 conv.kernel_size, conv.stride, conv.padding, conv.dilation)


def bn_eval_apply(bn, z, relu=False, rep=1, out=None):
    """Eval-mode BatchNorm3d (+ ReLU) (+ nearest T-repeat) of the raw tensor z as ONE affine pass with bn_affine's
    scale and bias — the un-fused form of the CMDA epilogues, taken under an EvalTape.  Its backward (sf_epilogue_bwd)
    leaves dL/dz in z's own buffer, where the producer's backward looks for it (as bn_train_apply does)."""
    sc, bi = bn_affine(bn)
    y = sfhip.affine(z, sc, bi, relu=relu, rep=rep, out=out)
    t = tape()
    if t is not None:
        t.record(lambda: sfhip.epilogue_bwd(t.grad_of(y), y, z, scale=sc, relu=relu, rep=rep))
    return y


def stem_geometry(conv, H, W):
    """(ph, pw, Wp) of the border-padded NDHWC4 input the stem convolution `conv` consumes for H x W frames."""
    kT, kH, kW = conv.kernel_size
    _, sH, sW = conv.stride
    pT, pH, pW = conv.padding
    Wo = (W + 2 * pW - kW) // sW + 1
    wp_need = max(W + 2 * pW, (Wo - 1) * sW + kW)
    return pH, pW, (wp_need + sW - 1) // sW * sW


def stem_conv_bn_relu(x, conv, bn, relu=True):
    """First convolution of a pathway straight from the caller's NCTHW clip (Cin <= 4).

    The clip is converted ONCE to NDHWC with channels padded to 4 and the H/W borders zero padded, so a
    (kT,kH,kW) conv with W-stride sW becomes a (kT,kH,1) conv over 'pixels' of sW*4 floats that consumes
    kW*4 CONTIGUOUS floats per tap: aligned 16-byte loads, no border predicate in H/W, and the K dimension
    is kT*kH taps x 4kW instead of kT*kH*kW taps x 16-padded 3 channels."""
    assert conv.groups == 1 and conv.in_channels <= 4 and conv.dilation == (1, 1, 1) and conv.stride[0] == 1
    kT, kH, kW = conv.kernel_size
    _, sH, sW = conv.stride
    pT, pH, pW = conv.padding
    N, C, T, H, W = x.shape
    Ho = (H + 2 * pH - kH) // sH + 1
    Wo = (W + 2 * pW - kW) // sW + 1
    wp_need = max(W + 2 * pW, (Wo - 1) * sW + kW)
    Wp = (wp_need + sW - 1) // sW * sW
    if isinstance(x, sfhip.PackedClip):  # produced by the GPU input step already in this layout
        if x.C != conv.in_channels:
            raise ValueError("a %d-channel PackedClip was handed to a stem that convolves %d channels" % (
                x.C, conv.in_channels))
        if (x.ph, x.pw, x.Wp) != (pH, pW, Wp):
            raise ValueError("PackedClip geometry (ph, pw, Wp) = %s does not match this stem's %s; pack it with "
                             "engine.stem_geometry(conv, H, W)" % ((x.ph, x.pw, x.Wp), (pH, pW, Wp)))
    if C == 1:  # grayscale clips: one float per pixel and the one-channel stem kernels, where they serve the conv
        t = tape()
        wants_grad = t is not None and isinstance(x, torch.Tensor) and id(x) in t.input_ids
        if not wants_grad and sfhip.stem1_accepts(H + 2 * pH, Wp, conv.out_channels, conv.kernel_size, conv.stride,
                                                  conv.dilation, conv.groups):
            return _stem1_conv_bn_relu(x, conv, bn, relu, (pH, pW, Wp))
        if isinstance(x, sfhip.PackedClip):  # out of the kernels' range: the padded route below, from the dense clip
            x = x.to_ncthw()
    if isinstance(x, sfhip.PackedClip):
        abuf = x.buf
    else:
        abuf = sfhip.from_ncthw(x, cpad=4, ph=pH, pw=pW, wp=Wp).buf
    view = Act(abuf.view(N, T, H + 2 * pH, Wp // sW, 4 * sW))

    def make():
        w = conv.weight
        w4 = torch.zeros((w.shape[0], 4, kT, kH, kW), dtype=torch.float32, device=w.device)
        w4[:, :C] = w
        cin = 4 * kW
        cin_pad = (cin + 15) // 16 * 16
        wp = torch.zeros((w.shape[0], kT * kH, cin_pad), dtype=torch.float32, device=w.device)
        wp[:, :, :cin] = w4.permute(0, 2, 3, 4, 1).reshape(w.shape[0], kT * kH, cin)
        return wp.contiguous()

    wp = _cached(conv, "_sf_wp_stem", _key(conv.weight), make)
    thw = (T + 2 * pT - kT + 1, Ho, Wo)
    if bn_unfused(bn):  # training mode, or frozen (eval mode) under a training tape
        want = bn.training and _plain_bn(bn) and bn.affine
        z = sfhip.conv(view, wp, (kT, kH, 1), (1, sH, 1), (pT, 0, 0), bias=conv.bias, cin=4 * kW, out_thw=thw,
                       stats=want)
        z, st = z if want else (z, None)

        def unpack(dwp):  # [Cout][kT*kH][kW*4 + c] -> [Cout, C, kT, kH, kW]
            co = dwp.shape[0]
            return dwp[:, :, :4 * kW].reshape(co, kT, kH, kW, 4)[..., :C].permute(0, 4, 1, 2, 3).contiguous()

        _record_conv(view, conv.weight, conv.bias, wp.shape, z, (kT, kH, 1), (1, sH, 1), (pT, 0, 0), (1, 1, 1),
                     x_needs_grad=False, cin=4 * kW, unpack=unpack, fold_kw=kW)
        _record_stem_input_grad(x, conv, z, view, (N, C, T, H, W), (pH, pW, Wp), Wo)
        return bn_apply(bn, z, relu=relu, conv_stats=st)
    scale, bias = bn_affine(bn, conv.bias)
    return sfhip.conv(view, wp, (kT, kH, 1), (1, sH, 1), (pT, 0, 0), scale=scale, bias=bias, relu=relu,
                      cin=4 * kW, out_thw=thw)


def _stem1_conv_bn_relu(x, conv, bn, relu, geom):
    """stem_conv_bn_relu for a one-channel clip (tensor [N,1,T,H,W] or one-channel PackedClip) on sf_stem1_fwd: the
    weights are read as the parameter holds them; training records the weight gradient (sf_stem1_wgrad) on the tape."""
    pH, pW, Wp = geom
    kT, pT = conv.kernel_size[0], conv.padding[0]
    buf = x.buf if isinstance(x, sfhip.PackedClip) else sfhip.ncthw1_pack(x, pH, pW, Wp)
    w = conv.weight.detach()
    if bn_unfused(bn):  # training mode, or frozen (eval mode) under a training tape
        z = sfhip.stem1_fwd(buf, w, pT, bias=conv.bias)
        _record_stem1_wgrad(buf, conv, z)
        return bn_apply(bn, z, relu=relu)
    scale, bias = bn_affine(bn, conv.bias)
    return sfhip.stem1_fwd(buf, w, pT, scale=scale, bias=bias, relu=relu)


def _record_stem1_wgrad(buf, conv, z):
    """dL/d(conv.weight) of the one-channel stem: its own step on the tape (the clip has no gradient on this route)."""
    t = tape()
    if t is None:
        return
    kT, pT = conv.kernel_size[0], conv.padding[0]

    def bwd():  # z's buffer holds dL/dz after the BN backward
        tgt = t.pgrad_target(conv.weight)
        if tgt is not None:
            sfhip.stem1_wgrad(buf, z, kT, pT, into=tgt)
        else:
            t.add_pgrad(conv.weight, sfhip.stem1_wgrad(buf, z, kT, pT))
        if conv.bias is not None:
            t.add_pgrad(conv.bias, _colsum(z))

    t.record(bwd)


def _record_stem_input_grad(x, conv, z, view, ncthw, geom, Wo):
    """dL/d(clip) when the caller asked for it (x.requires_grad: saliency / adversarial uses; train_net.py never
    does).  In the stem-trick layout a tap reads kW*4 contiguous floats = ceil(kW*4 / (4*sW)) whole pixels of 4*sW
    floats, so the stem IS an ordinary conv with kernel (kT, kH, KP) over pixels with 4*sW channels (weights
    re-arranged, zero where a tap's float index runs past kW*4) and its data gradient is the generic one; the clip's
    gradient is the interior (borders and the pad channel dropped) of that buffer."""
    t = tape()
    if t is None or not isinstance(x, torch.Tensor) or id(x) not in t.input_ids:
        return
    N, C, T, H, W = ncthw
    pH, pW, Wp = geom
    kT, kH, kW = conv.kernel_size
    _, sH, sW = conv.stride
    pT = conv.padding[0]
    pix = 4 * sW
    KP = (kW * 4 + pix - 1) // pix
    if view.W - KP + 1 != Wo:
        raise NotImplementedError("input gradient of a stem whose packed row is wider than its outputs need")
    idx = t.input_ids[id(x)]

    def make():  # [Cout, 3, kT, kH, kW] -> pixel-conv weight [Cout, pix, kT, kH, KP] -> data-gradient packing
        w = conv.weight
        w4 = torch.zeros((w.shape[0], kT, kH, KP * pix), dtype=torch.float32, device=w.device)
        w4[..., :kW * 4].view(w.shape[0], kT, kH, kW, 4)[..., :C] = w.permute(0, 2, 3, 4, 1)
        wpix = w4.view(w.shape[0], kT, kH, KP, pix).permute(0, 4, 1, 2, 3).contiguous()
        return sfhip.pack_conv_weight(wpix.transpose(0, 1).contiguous())

    def bwd():  # z's buffer holds dL/dz after the BN backward
        wtp = _cached_t(conv.weight, "_sf_wtp_stem", _key(conv.weight), make)
        dxp = sfhip.conv_dgrad(z, wtp, view, (kT, kH, KP), (1, sH, 1), (pT, 0, 0))
        full = dxp.buf.view(N, T, H + 2 * pH, Wp, 4)
        t.input_grads[idx] = full[:, :, pH:pH + H, pW:pW + W, :C].permute(0, 4, 1, 2, 3).contiguous()

    t.record(bwd)


def maxpool(x, kernel, stride, padding=(0, 0, 0), out_reserve=(0, 0)):
    """MaxPool3d (+ its backward on the tape)."""
    t = tape()
    if t is None:
        return sfhip.pool(x, kernel, stride, padding, out_reserve=out_reserve)
    y, arg = sfhip.pool(x, kernel, stride, padding, out_reserve=out_reserve, want_arg=True)
    if t is not None:
        def bwd():
            dx, acc = t.grad_dst(x)  # first writer of x's gradient: write, no zero fill / read
            # the forward's winner map: no x / y reads, no tie search (else: the search form)
            if arg is not None and sfhip.maxpool_bwd_arg(x, arg, t.grad_of(y), dx, kernel, stride, padding,
                                                         overwrite=not acc):
                return
            sfhip.maxpool_bwd(x, y, t.grad_of(y), dx, kernel, stride, padding, overwrite=not acc)

        t.record(bwd)
    return y


_GRAD_SINK = False


def set_grad_sink(enabled):
    """Opt-in fast path for the training step: parameter gradients are ACCUMULATED IN PLACE into the parameters'
    existing .grad tensors by the backward kernels themselves (conv weight gradients: partial-sum + un-pack +
    accumulate in one launch; BatchNorm dgamma/dbeta: inside the reduction's final kernel) instead of being handed
    to autograd, which would add one temporary, one copy and one accumulate launch per parameter.  Use it with
    pre-allocated gradients (utils.distributed.FlatGradients binds every .grad to one flat buffer).  Autograd
    hooks on the parameters (DistributedDataParallel) do NOT fire for sunk gradients: leave it off under DDP —
    run_model raises for a model that build_model wrapped in DistributedDataParallel while the sink is on."""
    global _GRAD_SINK
    _GRAD_SINK = bool(enabled)


class TapedForward(torch.autograd.Function):
    """The whole HIP forward as ONE autograd node: forward records the tape, backward replays it and hands
    the parameter gradients back to autograd (so .grad accumulation and DDP's all-reduce hooks work as for
    any module).  Activations never become autograd tensors."""

    @staticmethod
    def forward(ctx, model, n_in, bboxes, *args):
        inputs, params = list(args[:n_in]), args[n_in:]
        t = Tape()
        t.model = model
        t.input_ids = {id(x): i for i, x in enumerate(inputs)
                       if isinstance(x, torch.Tensor) and ctx.needs_input_grad[3 + i]}
        with taping(t):
            out = model._forward_impl(inputs) if bboxes is None else model._forward_impl(inputs, bboxes)
        if t.out_act is None:
            raise RuntimeError("the head did not register its logits on the tape")
        ctx.tape = t
        ctx.params = params
        ctx.n_in = n_in
        return out

    @staticmethod
    def backward(ctx, dout):
        t = ctx.tape
        if _GRAD_SINK:  # accumulate into the existing .grad tensors ourselves; autograd gets None for those
            t.sink = {p: p.grad for p in ctx.params if p.grad is not None and p.grad.dtype == torch.float32}
        with torch.no_grad(), taping(None):
            g = t.grad_of(t.out_act)
            g.buf.copy_(dout.reshape(g.buf.shape))
            t.backward()
        sink = t.sink or {}
        grads = tuple(None if p in sink else t.pgrads.get(p) for p in ctx.params)
        gin = tuple(t.input_grads.get(i) for i in range(ctx.n_in))
        if any(ctx.needs_input_grad[3 + i] and gin[i] is None for i in range(ctx.n_in)):
            raise NotImplementedError("dL/d(input) was requested for an input this model's stem does not "
                                      "differentiate (PackedClip inputs / non-stem consumers)")
        ctx.tape = None
        return (None, None, None) + gin + grads


def run_model(model, x, bboxes=None):
    """model.forward body shared by all model classes: taped when training with grad enabled.  bboxes: the detection
    head's [K, 5] boxes (models built with DETECTION.ENABLE), handed to _forward_impl; never an autograd input."""
    global _NBT
    outer, _NBT = _NBT, []
    # collective-carrying layers (Sync-BN over > 1 local rank): one stream for this model only.  The decision depends on
    # the process group's state, so the cache is keyed on it (a forward before init_process_group must not pin False)
    from slowfast.utils import distributed as du
    local_size = du.get_local_size()
    cached = model.__dict__.get("_sf_serial_streams")
    if cached is None or cached[0] != local_size:
        serial = local_size > 1 and any(getattr(m, "_sf_collective", False) for m in model.modules())
        model.__dict__["_sf_serial_streams"] = (local_size, serial)
        if serial and OVERLAP_PATHS:
            print("[sfhip] %s holds Sync-BN layers over %d local ranks: its pathways run on one stream (collectives "
                  "stay in program order)" % (type(model).__name__, local_size))
    else:
        serial = cached[1]
    outer_serial, _tls.serial = getattr(_tls, "serial", False), serial
    outer_cap = getattr(_tls, "capturing", False)
    _tls.capturing = bool(torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())
    try:
        if model.training and torch.is_grad_enabled():
            if _GRAD_SINK and getattr(model, "_sf_ddp_wrapped", False):
                raise RuntimeError("engine.set_grad_sink(True) bypasses autograd's gradient hooks, which "
                                   "DistributedDataParallel's all-reduce depends on: switch the sink off, or use "
                                   "utils.distributed.FlatGradients on the unwrapped model")
            params = [p for p in model.parameters()]
            repack_all(model)
            boxes = bboxes.detach() if isinstance(bboxes, torch.Tensor) else bboxes
            return TapedForward.apply(model, len(x), boxes, *x, *params)
        return model._forward_impl(x) if bboxes is None else model._forward_impl(x, bboxes)
    finally:
        if x and hasattr(x[0], "device") and x[0].device.type == "cuda":
            join_pending(x[0].device)  # a fusion whose join was deferred and that no later region picked up
        _tls.serial = outer_serial
        _tls.capturing = outer_cap
        counters, _NBT = _NBT, outer
        if counters:
            with torch.no_grad():
                torch._foreach_add_(counters, 1)


def copy_channels(x, out, out_cmul=1):
    """out[.., out.coff + c*out_cmul] = x[.., c] (+ the gather on the tape)."""
    sfhip.copy_channels(x, out, out_cmul=out_cmul)
    t = tape()
    if t is not None:
        t.record(lambda: sfhip.gather_add(t.grad_of(out), out_cmul, t.grad_of(x), accumulate=True))
    return out


def add_into(a, res, out):
    """out = a + res (elementwise, channel slices), taped: both inputs receive dL/dout."""
    sfhip.affine(a, res=res, out=out)
    t = tape()
    if t is not None:
        def bwd():
            g = t.grad_of(out)
            sfhip.axpy(g, t.grad_of(a), 1.0, accumulate=True)
            sfhip.axpy(g, t.grad_of(res), 1.0, accumulate=True)
        t.record(bwd)
    return out


def avgpool(x, kernel, stride, padding):
    """nn.AvgPool3d(kernel, stride, padding) with count_include_pad=True: a depthwise conv whose taps are all
    1/|kernel| (zero padding == counting the pad).  Taped: the data gradient is the transposed gather."""
    taps = kernel[0] * kernel[1] * kernel[2]
    # keyed on the issuing stream too: a constant created inside a run_paths region must not be shared with the
    # other stream before the region's join
    key = ("avgpool", taps, x.C, str(x.buf.device), torch.cuda.current_stream(x.buf.device).cuda_stream)
    w = _PCACHE.get(key)
    if w is None:
        w = torch.full((taps, x.C), 1.0 / taps, dtype=torch.float32, device=x.buf.device)
        _PCACHE[key] = w
    y = sfhip.dwconv(x, w, kernel, stride, padding)
    t = tape()
    if t is not None:
        t.record(lambda: sfhip.dwconv_dgrad(x, t.grad_of(y), w, kernel, stride, padding, t.grad_of(x)))
    return y


def global_mean(x, out=None):
    """[N,T,H,W,C] -> [N,1,1,1,C] mean over T,H,W (taped)."""
    pooled = sfhip.tmax_mean(x, 1)
    a = Act(pooled.view(x.N, 1, 1, 1, x.C))
    res = sfhip.copy_channels(a, out) if out is not None else a
    t = tape()
    if t is not None:
        def bwd():
            g = t.grad_of(res)
            v = g.buf.view(g.N, g.cs)[:, g.coff:g.coff + g.C].contiguous()
            sfhip.bcast_add(t.grad_of(x), v, 1.0 / float(x.T * x.H * x.W))
        t.record(bwd)
    return res


def small_torch_op(inputs, params, fn):
    """A parameter-sized sub-graph ([N, C] tensors: SE excitation, GhostNet's conv_head on pooled features)
    evaluated with torch ops; on the tape its backward is torch.autograd.grad over the tiny graph.
    inputs: list of Acts whose views are [N,1,1,1,C]; fn(list of [N,C] tensors) -> [N,K] tensor.
    Returns an Act [N,1,1,1,K]."""
    t = tape()
    flat = [a.buf.view(a.N, a.cs)[:, a.coff:a.coff + a.C] for a in inputs]
    if t is None:
        with torch.no_grad():
            y = fn([f for f in flat])
        return Act(y.contiguous().view(y.shape[0], 1, 1, 1, y.shape[1]))
    with torch.enable_grad():
        leaves = [f.detach().clone().requires_grad_(True) for f in flat]
        y = fn(leaves)
    out = Act(y.detach().contiguous().view(y.shape[0], 1, 1, 1, y.shape[1]))

    def bwd():
        g = t.grad_of(out).buf.view(y.shape)
        grads = torch.autograd.grad(y, leaves + list(params), g, allow_unused=True)
        for a, ga in zip(inputs, grads[:len(leaves)]):
            if ga is not None:
                ga_act = Act(ga.contiguous().view(a.N, 1, 1, 1, a.C))
                sfhip.axpy(ga_act, t.grad_of(a), 1.0, accumulate=True)
        for p, gp in zip(params, grads[len(leaves):]):
            if gp is not None:
                t.add_pgrad(p, gp)

    t.record(bwd)
    return out
