#!/usr/bin/env python3
"""bench.py — clips/sec of the SlowFast hot path on MI355X (one process per GPU).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload dual|slowfast|ghostnet|shufflenetv2] [--full]
                    [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: set up, warm up (the W steps, then on to a steady state), time
exactly K steps, write the last timed step's outputs (--dump-outputs) and print the JSON line.  Everything else this
file measures or checks runs only with --full: the clock probe, the eval-forward figure, the dominant-kernel trace
(roofline, kernel_family_ms_per_step, launch_bound), the CPU baseline with the parity fields and the parity gate, the
gradient hash of the canonical state.

--dump-outputs DIR: after the timed steps, what the LAST timed step computed, as DIR/<name>.npy (float32): train =
loss, logits, and the parameters, their gradients and the float buffers (BN running statistics) after that step, each
concatenated in named_parameters / named_buffers order (a fixed, seeded sample of DUMP_SAMPLE elements where longer);
eval = the output probabilities.  In train mode the timed steps start from the seeded state (parameters, buffers, zero
momentum, seeded dropout generator) whatever number of steps the warm-up ran, so the same arguments give the same
outputs from run to run and build to build.

Called directly with --gpus N > 1 (no launcher in the environment) the process starts N children itself, one per
GPU, BEFORE any GPU call (the reference spawns its ranks the same way: utils/misc.py:275-303 launch_job ->
torch.multiprocessing.spawn, utils/multiprocessing.py:9-61), waits for them, lets rank 0 print the JSON line and
exits non-zero if any child did.  Under torch.distributed.run it is one of the ranks, as before.

--mode train (default): a "step" is one training iteration of the reference's loop (tools/train_net.py:78-96)
over one batch of synthetic clips already resident in HBM (fp32 NCTHW): train-mode forward (batch-statistics
BN, dropout), cross-entropy, backward through every kernel, ONE all-reduce of the flat gradient buffer across
ranks (RCCL) and an SGD(momentum, weight-decay) update.  --mode eval: one eval-mode forward pass (inference).  Default workload =
BASELINE.json's metric config: SlowFastDualAttention 8x8 R50 + CMDA, 224^2, 8 clips per GPU (configs[2];
at N GPUs configs[3]: global batch 8N).  Parameters are the de-degenerated seeded fill of
tests/golden/paramgen.py (gamma != 0, non-zero final BNs) so no part of the network is a no-op.

Prints ONE JSON line (rank 0) with the driver's contract fields plus, with --full,
  roofline:     the dominant kernel (flash attention, C=32, N=25088) — algorithmic FLOPs per launch /
                its HIP-event duration measured around every launch inside the timed region, vs the dense
                fp32 MFMA peak (157.3 TFLOP/s);
  cpu_baseline: the oracle (torch CPU restatement of the reference) timed on this box's host cores (N=1 only,
                bounded sample: batch 1 of the SAME workload — train-mode forward + CE + autograd backward in train
                mode — 3 warm-up + 5 timed iterations, median; `cores` = threads used, `host_cores` = os.cpu_count());
  fwd_max_rel_err / fwd_logits_max_rel_err / bwd_max_rel_err: the HIP path against that oracle run on the same
                full-size clip (eval probabilities, pre-activation logits; train-mode loss and every parameter
                gradient's relative L2 error, worst and median);
and in every run
  n_ranks_seen: an all-reduce of ones over the job's process group (RCCL) — the ranks that really took part.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "efficient-slowfast_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

WORKLOADS = {
    "dual": ("SLOWFAST_DUAL_8x8_R50.yaml", 8, "SlowFastDualAttention 8x8 R50 + CMDA, 224^2, T=32 alpha=4"),
    "slowfast": ("SLOWFAST_8x8_R50.yaml", 8, "SlowFast 8x8 R50 (no attention), 224^2, T=32 alpha=4"),
    "ghostnet": ("SLOWFAST_GHOSTNET_32x2.yaml", 2, "SlowFastGhostNet w2.0 + CMDA, 32x2, 224^2"),
    "shufflenetv2": ("SLOWFAST_SHUFFLENETV2_4x16.yaml", 2, "SlowFastShuffleNetV2 w0.25, 4x16, 32^2"),
}
PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense f32-in MFMA = vector peak
PEAK_SCLK_MHZ = 2400.0        # MI355X_MICROARCH.md peak engine clock (pp_dpm_sclk top level on the pool's boxes): what the peaks above assume
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA
PARAM_SEED = 7
DUMP_SAMPLE = 1 << 22         # --dump-outputs: elements kept of a longer concatenated output (16 MB of float32 each)
DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: all files together


def build(workload, device):
    from paramgen import fill_state_dict
    from slowfast.config.defaults import get_cfg
    from slowfast.models import build_model
    yaml_name, batch, desc = WORKLOADS[workload]
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", yaml_name))
    cfg.NUM_GPUS = 1
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = build_model(cfg)
    fill_state_dict(model.state_dict(), PARAM_SEED)
    return cfg, model.eval(), batch, desc


def synthetic_clips(cfg, batch, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t, s, a = cfg.DATA.NUM_FRAMES, cfg.DATA.CROP_SIZE, cfg.SLOWFAST.ALPHA
    fast = torch.randn(batch, 3, t, s, s, generator=g)
    idx = torch.linspace(0, t - 1, t // a).long()  # pack_pathway_output (datasets/utils.py:93-104)
    slow = fast.index_select(2, idx)
    return [slow.to(device), fast.to(device)]


def oracle_hparams(cfg):
    from oracle import slowfast_oracle as oracle
    return oracle.default_hparams(
        alpha=cfg.SLOWFAST.ALPHA, beta_inv=cfg.SLOWFAST.BETA_INV, depth=cfg.RESNET.DEPTH,
        width_per_group=cfg.RESNET.WIDTH_PER_GROUP, num_groups=cfg.RESNET.NUM_GROUPS,
        fusion_kernel=cfg.SLOWFAST.FUSION_KERNEL_SZ,
        spatial_strides=[s[0] for s in cfg.RESNET.SPATIAL_STRIDES],
        spatial_dilations=[s[0] for s in cfg.RESNET.SPATIAL_DILATIONS],
        num_block_temp_kernel=[list(x) for x in cfg.RESNET.NUM_BLOCK_TEMP_KERNEL],
        num_frames=cfg.DATA.NUM_FRAMES, crop_size=cfg.DATA.CROP_SIZE, num_classes=cfg.MODEL.NUM_CLASSES,
        short_cycle=bool(cfg.MULTIGRID.SHORT_CYCLE), head_act=cfg.MODEL.HEAD_ACT,
        width_multi=cfg.SLOWFAST.WIDTH_MULTI)


def cpu_baseline(workload, cfg, model, train, device=None, hip_train_step=None, parity_only=False):
    """The oracle on the host cores, batch 1 (dense attention needs ~6 GB per clip, ~3x that with autograd), timed as
    SURVEY §8d asks: thread count chosen on the SAME workload that is reported (one iteration per candidate), then
    3 warm-up + 5 timed iterations at that count, median.  The same oracle runs are the checker of the metric's second
    half: returns (cpu_baseline dict, parity dict) — the HIP eval forward (probabilities and logits) and, in train
    mode, the HIP training step (loss, logits, every parameter's gradient) against the oracle on that clip.
    hip_train_step(xs, label) -> (loss, logits, {param name: grad}) runs the HIP model on the clip (dropout off)."""
    from oracle import slowfast_oracle as oracle
    hp = oracle_hparams(cfg)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    # one clip of the benchmark shape — except cfg #1 (32^2 clips: its last stages are 1 x 1 frames, so ONE clip leaves
    # 4 values per channel for the batch statistics and every gradient behind them is ill-conditioned): its own 2 clips
    nclip = 2 if workload == "shufflenetv2" else 1
    xs = synthetic_clips(cfg, nclip, "cpu", 1)
    name = cfg.MODEL.MODEL_NAME
    label = torch.arange(nclip, dtype=torch.long) % cfg.MODEL.NUM_CLASSES
    keep = {}

    def iteration(keep_grads=False, dtype=torch.float32):
        if not train:
            return oracle.forward(name, sd, xs, hp)["out"]
        sdr = {k: (v.to(dtype).clone().requires_grad_(True) if v.dtype == torch.float32 and "running" not in k
                   else (v.to(dtype) if v.dtype == torch.float32 else v)) for k, v in sd.items()}
        acts = oracle.FORWARDS[name](sdr, [x.to(dtype).clone() for x in xs], hp, training=True)
        loss = torch.nn.functional.cross_entropy(acts["out"], label)
        loss.backward()
        if keep_grads:
            keep["loss"], keep["logits"] = float(loss.detach()), acts["out"].detach()
            keep["grads"] = {k: v.grad for k, v in sdr.items() if getattr(v, "grad", None) is not None}
        return None

    # ---- parity at the full size (BASELINE.json metric: "fwd max|delta| vs ref"), eval forward first: the training
    #      forward below moves the HIP model's running statistics
    parity = {}
    if device is not None:
        torch.set_num_threads(min(os.cpu_count() or 1, 32))
        ref = oracle.forward(name, sd, xs, hp)
        was_training = model.training
        model.eval()
        with torch.no_grad():
            got = model([x.to(device) for x in xs]).cpu()
        model.train(was_training)
        parity["fwd_max_rel_err"] = float((got - ref["out"]).abs().max() / ref["out"].abs().max())
        if train and hip_train_step is not None:
            # the HIP step first, recording its ReLU masks and max-pool winners; the oracle then differentiates the SAME
            # piecewise-linear function (tests/_masks.py) — without that the comparison measures mask flips (a 3e-2
            # floor that does not shrink with size), not the backward arithmetic
            import _masks
            with _masks.capture() as masks:
                loss, logits, grads = hip_train_step([x.to(device) for x in xs], label.to(device))
            m32 = masks.fork()   # (a replay cursor: every oracle run starts from the first captured layer)
            with _masks.inject(m32):
                iteration(keep_grads=True)
            rl = keep["logits"]
            parity["fwd_logits_max_rel_err"] = float((logits.cpu() - rl).abs().max() / rl.abs().max())
            parity["train_loss_abs_err"] = abs(float(loss) - keep["loss"])
            # analytically zero gradients (tests/_zero_grads.py: value / key bias of SpatialAttention, ECA's 3-tap
            # weight, BN biases that only meet 1x1x1 convs + batch-statistics BNs) hold rounding noise on both sides:
            # not part of the relative statistic, bounded absolutely (reported as bwd_zero_class_*)
            import _zero_grads
            noise, gmax = _zero_grads.split(keep["grads"])
            errs = []
            for k, g in keep["grads"].items():
                if k in grads and float(g.norm()) > 0 and k not in noise:
                    errs.append((float((grads[k].cpu() - g).norm() / g.norm()), k))
            errs.sort()
            parity["bwd_zero_class_params"] = len(noise)
            if workload in _zero_grads.EXPECTED:  # (asserted in tests/test_fullsize_gpu.py; here only reported)
                parity["bwd_zero_class_params_expected"] = _zero_grads.EXPECTED[workload]
            parity["bwd_zero_class_max_abs_err_over_gmax"] = max(
                [float((grads[k].cpu() - keep["grads"][k]).norm()) / gmax for k in noise if k in grads] or [0.0])
            parity["bwd_max_rel_err"] = errs[-1][0]
            parity["bwd_median_rel_err"] = errs[len(errs) // 2][0]
            parity["bwd_worst_param"] = errs[-1][1]
            parity["bwd_params_compared"] = len(errs)
            parity["bwd_masks_injected"] = {"relu": m32.used, "max_pool": m32.pool_used,
                                            "missed": len(m32.missed)}
            # the same step once more with the oracle in fp64 (same clip, parameters, masks): what the fp32 oracle itself
            # is off by — the reference's own rounding noise, the floor of every number above (profiles/
            # r06_oracle_conditioning_dual.txt: median 2.3e-4, 9.9e-4 on s4_fuse's key conv) — and the HIP gradients
            # against that (near-)exact result, parameter by parameter
            if os.environ.get("SF_BENCH_FP64_CHECK", "1") != "0":
                try:
                    g32 = keep["grads"]
                    m64 = masks.fork()
                    with _masks.inject(m64):
                        iteration(keep_grads=True, dtype=torch.float64)
                    parity["fp64_masks_injected"] = {"relu": m64.used, "max_pool": m64.pool_used, "missed": len(m64.missed)}
                    g64 = keep["grads"]
                    e_hip, e_ref = [], []
                    for k, g in g64.items():
                        if k in grads and k in g32 and float(g.norm()) > 0 and k not in noise:
                            e_hip.append((float((grads[k].cpu().double() - g).norm() / g.norm()), k))
                            e_ref.append((float((g32[k].double() - g).norm() / g.norm()), k))
                    e_hip.sort()
                    e_ref.sort()
                    parity["fwd_logits_max_rel_err_vs_fp64"] = float(
                        (logits.cpu().double() - keep["logits"]).abs().max() / keep["logits"].abs().max())
                    parity["bwd_median_rel_err_vs_fp64"] = e_hip[len(e_hip) // 2][0]
                    parity["bwd_max_rel_err_vs_fp64"] = e_hip[-1][0]
                    parity["bwd_worst_param_vs_fp64"] = e_hip[-1][1]
                    parity["oracle_fp32_vs_fp64_bwd_median"] = e_ref[len(e_ref) // 2][0]
                    parity["oracle_fp32_vs_fp64_bwd_max"] = e_ref[-1][0]
                    parity["oracle_fp32_vs_fp64_worst_param"] = e_ref[-1][1]
                except (RuntimeError, MemoryError) as e:  # e.g. a host without the ~40 GB the fp64 attention graphs need
                    parity["fp64_check_skipped"] = "%s: %s" % (type(e).__name__, str(e)[:120])
            keep.clear()
    if parity_only:   # the checker alone (the trained-state comparison): nothing is timed
        return None, parity
    # ATen's CPU conv/softmax stop scaling (and collapse when oversubscribed: 256 SMT threads ran 350x slower
    # than 8 cores) well below this box's core count: one iteration of the reported workload per candidate count
    best = None
    for threads in sorted({min(os.cpu_count() or 1, t) for t in (16, 32, 64)}):
        torch.set_num_threads(threads)
        t0 = time.time()
        iteration()
        dt = time.time() - t0
        if best is None or dt < best[0]:
            best = (dt, threads)
    threads = best[1]
    torch.set_num_threads(threads)
    warm, timed = 3, 5
    for _ in range(warm):
        iteration()
    times = []
    for _ in range(timed):
        t0 = time.time()
        iteration()
        times.append(time.time() - t0)
    dt = sorted(times)[len(times) // 2]
    what = ("train-mode forward + CE + autograd backward" if train else "eval forward")
    sample = "%s, batch %d; %d threads (fastest of 16/32/64 on one iteration of this workload), %d warm-up + %d timed " \
             "iterations, median (min %.2f s, max %.2f s)" % (what, nclip, threads, warm, timed, min(times), max(times))
    return ({"value": round(nclip / dt, 4), "unit": "clips/s", "cores": threads, "host_cores": os.cpu_count(),
             "kind": "port",
             "sample": "oracle (torch CPU restatement of the reference), same model / clip shape: " + sample}, parity)


GATED = (("fwd_max_rel_err", 1e-3), ("fwd_logits_max_rel_err", 1e-3), ("bwd_median_rel_err", 1e-3))


def parity_gate(res):
    """The violations that make bench.py exit 3 (the line is printed either way): the SEEDED state's forward — eval
    probabilities and train-mode logits — and its typical parameter gradient against the oracle, north_star's 1e-3.
    Deterministic figures with a 4x margin (2.2e-6, 4.5e-6, 2.6e-4 on cfg #3).  Not gated: bwd_max_rel_err (single
    ill-conditioned parameters sit at the tolerance on the oracle's own fp32-vs-fp64 error) and the trained
    state's *_after_steps fields (they depend on how many steps a box's steady-state search ran)."""
    out = []
    for k, lim in GATED:
        if k in res and not (res[k] <= lim):   # (NaN fails)
            out.append("%s = %.3e > %.0e" % (k, res[k], lim))
    return out


def make_train_step(model, clips, labels, overlap_allreduce=True, lr=1e-3):
    """The benchmark's training step (the reference loop: tools/train_net.py:78-96) as a closure over resident clips:
    zero the flat gradient buffer, train-mode forward, cross-entropy, backward through the tape (parameter gradients
    accumulated by the kernels straight into the flat buffer), ONE all-reduce of that buffer, torch.optim.SGD step.
    Returns (step, flat, opt); step() returns the loss tensor and leaves the step's logits (detached) in step.logits
    (a capture's static output when the step is captured).  tests/test_graph_train_gpu.py replays exactly this
    closure from a hipGraph against its eager form.  A captured graph of it is replayed with engine.replay(graph) (or
    followed by engine.parameters_changed()): the replayed optimizer kernel does not run torch's optimizer hooks."""
    from slowfast.models import engine
    from slowfast.utils.distributed import FlatGradients
    model.train()
    flat = FlatGradients(model.parameters())
    engine.set_grad_sink(os.environ.get("SF_NO_GRAD_SINK") != "1")  # backward kernels accumulate straight into the flat gradient buffer
    if overlap_allreduce:
        # res5 + head, then res4 (+ s4_fuse): 85 % of the gradient bytes, final ~10 ms into the backward pass —
        # their all-reduce runs on its own stream under the rest of the backward; the remainder after it
        flat.overlap_with_backward(model, boundaries=("s5", "s4"))
    # torch's SGD (the reference: models/optimizer.py:53-60 torch.optim.SGD with momentum + weight decay); fused=True is
    # torch's single multi-tensor kernel per step instead of its four foreach passes (SF_SGD_FUSED=0: the foreach form)
    sgd = dict(lr=lr, momentum=0.9, weight_decay=1e-4)
    opt = None
    if os.environ.get("SF_SGD_FUSED", "1") != "0":
        try:
            opt = torch.optim.SGD(model.parameters(), fused=True, **sgd)
        except (TypeError, RuntimeError):
            opt = None
    if opt is None:
        opt = torch.optim.SGD(model.parameters(), **sgd)  # torch's default: the foreach implementation

    def step():
        flat.zero()
        logits = model([clips[0], clips[1]])
        step.logits = logits.detach()
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        flat.all_reduce_mean()      # ONE collective per step over RCCL / xGMI (no-op at world 1)
        opt.step()
        flat.rebind()
        return loss

    step.logits = None
    return step, flat, opt


def _dump_sample(v, seed):
    """v (1-D device tensor) whole when it has at most DUMP_SAMPLE elements, else DUMP_SAMPLE of them at fixed,
    seeded positions (the same for every run on the same model)."""
    n = v.numel()
    if n <= DUMP_SAMPLE:
        return v
    idx = np.sort(np.random.default_rng(seed).choice(n, DUMP_SAMPLE, replace=False))
    return v[torch.from_numpy(idx).to(v.device)]


def dump_outputs(out_dir, arrays):
    """--dump-outputs: {name: tensor} -> out_dir/<name>.npy as float32, at most DUMP_LIMIT_BYTES in all."""
    host = {k: np.ascontiguousarray(v.detach().float().cpu().numpy(), dtype=np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    assert total <= DUMP_LIMIT_BYTES, "outputs of %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    print("[bench] wrote %d outputs (%.1f MB) to %s" % (len(host), total / 2.0 ** 20, out_dir), file=sys.stderr)


def train_outputs(model, loss, logits):
    """What a caller of the training step receives from its last run: the loss, the logits, and the model the step
    left behind — parameters, their gradients and the float buffers, each concatenated in named order (sampled where
    longer than DUMP_SAMPLE)."""
    params = [p for _, p in model.named_parameters()]
    grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
    bufs = [b for _, b in model.named_buffers() if b.is_floating_point()]
    cat = lambda ts: torch.cat([t.detach().reshape(-1).float() for t in ts]) if ts else torch.zeros(0)  # noqa: E731
    return {"loss": loss.detach().reshape(1), "logits": logits,
            "params": _dump_sample(cat(params), 1), "grads": _dump_sample(cat(grads), 2),
            "buffers": _dump_sample(cat(bufs), 3)}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _parse_cpulist(txt):
    cpus = set()
    for part in txt.strip().split(","):
        if not part:
            continue
        a, _, b = part.partition("-")
        cpus.update(range(int(a), int(b or a) + 1))
    return cpus


def _fmt_cpulist(cpus):
    """[0, 1, 2, 3, 8, 9] -> '0-3,8-9'"""
    out, i = [], 0
    cpus = sorted(cpus)
    while i < len(cpus):
        j = i
        while j + 1 < len(cpus) and cpus[j + 1] == cpus[j] + 1:
            j += 1
        out.append(str(cpus[i]) if i == j else "%d-%d" % (cpus[i], cpus[j]))
        i = j + 1
    return ",".join(out)


def _visible_ordinals(n):
    """Physical ordinal of HIP device r for r < n under HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES
    / GPU_DEVICE_ORDINAL (numeric lists; they compose: ROCR filters what HIP then indexes), or None when a list is not
    numeric (UUIDs) or too short — the caller then does not guess."""
    phys = None
    for var in ("ROCR_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is None or v.strip() == "":
            continue
        try:
            lst = [int(x) for x in v.split(",") if x.strip() != ""]
        except ValueError:
            return None
        if phys is None:
            phys = lst
        else:
            if any(k >= len(phys) or k < 0 for k in lst):
                return None
            phys = [phys[k] for k in lst]
    if phys is None:
        return list(range(n))
    return phys[:n] if len(phys) >= n else None


def gpu_numa_nodes(n, sysfs="/sys"):
    """NUMA node of HIP devices 0 .. n-1 WITHOUT touching the GPU, or None per device where sysfs does not say.  HIP
    enumerates the KFD topology's GPU nodes (simd_count > 0) in node order; a node's `domain` and `location_id`
    (bus << 8 | device << 3 | function) are its PCI address, whose numa_node file names the host node.  (DRM render
    minors are NOT used: they need not be contiguous or ordered like HIP ordinals, and a BMC's VGA device takes one.)"""
    ords = _visible_ordinals(n)
    if ords is None:
        return [None] * n
    gpus = []
    top = os.path.join(sysfs, "class/kfd/kfd/topology/nodes")
    try:
        ids = sorted(int(d) for d in os.listdir(top) if d.isdigit())
    except OSError:
        return [None] * n
    for d in ids:
        props = {}
        try:
            with open(os.path.join(top, str(d), "properties")) as f:
                for line in f:
                    kv = line.split()
                    if len(kv) == 2:
                        props[kv[0]] = kv[1]
            if int(props.get("simd_count", "0")) <= 0:
                continue  # a CPU node
            loc, dom = int(props["location_id"]), int(props.get("domain", "0"))
        except (OSError, ValueError, KeyError):
            gpus.append(None)
            continue
        addr = "%04x:%02x:%02x.%d" % (dom, (loc >> 8) & 0xff, (loc >> 3) & 0x1f, loc & 7)
        try:
            with open(os.path.join(sysfs, "bus/pci/devices", addr, "numa_node")) as f:
                node = int(f.read().strip())
            gpus.append(node if node >= 0 else None)
        except (OSError, ValueError):
            gpus.append(None)
    return [gpus[o] if 0 <= o < len(gpus) else None for o in ords]


def rank_cpu_sets(n, sysfs="/sys"):
    """CPUs for each of n ranks of this node, WITHOUT touching the GPU: the CPUs of the NUMA node GPU r hangs off
    (gpu_numa_nodes) shared evenly between the ranks on that node; an even split of the allowed CPUs where sysfs does not
    say or the visibility variables cannot be followed.  The launcher threads of 8 ranks otherwise wander over one
    host.  -> [(node or -1, cpus)]"""
    allowed = sorted(os.sched_getaffinity(0))
    nodes = [-1 if k is None else k for k in gpu_numa_nodes(n, sysfs)]
    out = []
    for r in range(n):
        cpus = None
        if nodes[r] >= 0:
            try:
                with open(os.path.join(sysfs, "devices/system/node/node%d/cpulist" % nodes[r])) as f:
                    on_node = sorted(_parse_cpulist(f.read()) & set(allowed))
                peers = [q for q in range(n) if nodes[q] == nodes[r]]
                share = len(on_node) // len(peers)
                if share >= 1:
                    i = peers.index(r)
                    cpus = on_node[i * share:(i + 1) * share]
            except (OSError, ValueError):
                cpus = None
        if not cpus:
            share = max(1, len(allowed) // n)
            cpus = allowed[r * share:(r + 1) * share] or allowed
            nodes[r] = -1
        out.append((nodes[r], cpus))
    return out


def spawn_ranks(n, argv):
    """Start n copies of this script, one per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their environment:
    what torch.distributed.run would set), wait for all of them and return the exit code: 0 only if every rank
    exited 0.  Rank 0 inherits stdout (its JSON line is this command's); when a rank fails the others are stopped
    (exactly the PIDs started here).  The parent never initialises the GPU."""
    import subprocess
    port = _free_port()
    procs = []
    cpu_sets = rank_cpu_sets(n)
    for r, (node, cpus) in enumerate(cpu_sets):
        print("[bench] rank %d: %s, CPUs %s" % (r, "NUMA node %d" % node if node >= 0 else "no NUMA hint (even split)",
                                               _fmt_cpulist(cpus)), file=sys.stderr)
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, min(len(cpu_sets[r][1]), (os.cpu_count() or 8) // n))))
        # each rank pins itself (before its first GPU call) to the CPUs next to its GPU: main() applies SF_RANK_CPUS
        env.setdefault("SF_RANK_CPUS", ",".join(str(c) for c in cpu_sets[r][1]))
        env.setdefault("SF_RANK_NUMA", str(cpu_sets[r][0]))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                print("[bench] rank %d exited with %d: stopping the other ranks" % (procs.index(p), code),
                      file=sys.stderr)
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    return rc


def gpu_hwmon_dir(device_index, sysfs="/sys"):
    """hwmon directory (sclk `freq1_input` in Hz, package power `power1_input` in uW) of HIP device `device_index`, by
    its PCI address; the only GPU hwmon of the box when torch does not expose the address; None when there is none."""
    import glob
    cands = []
    try:
        pr = torch.cuda.get_device_properties(device_index)
        addr = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        cands = glob.glob(os.path.join(sysfs, "bus/pci/devices", addr, "hwmon/hwmon*"))
    except (AttributeError, RuntimeError):
        cands = []
    if not cands:
        every = [d for d in glob.glob(os.path.join(sysfs, "class/drm/card*/device/hwmon/hwmon*"))
                 if os.path.exists(os.path.join(d, "freq1_input"))]
        cands = every if len(every) == 1 else []
    cands = [d for d in cands if os.path.exists(os.path.join(d, "freq1_input"))]
    return cands[0] if cands else None


class ClockSampler:
    """Shader clock and package power of one GPU, read from its hwmon files every `period` s by a daemon thread while
    a few further steps run right after the timed region (inside it the reads were free on most boxes and cost
    3.6 ms per step on one with a slow host).  summary() -> the `clocks` block of the JSON line, or None when the box exposes no hwmon.  Why it is
    there: the step is clock limited — the part sustains ~2.2 of its 2.4 GHz under this load (profiles/
    r06_power_during_step.txt) and the rooflines of this file are quoted at the peak clock."""

    def __init__(self, hwmon, period=0.05):
        import threading
        self.dir, self.period, self.sclk, self.power = hwmon, period, [], []
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True) if hwmon else None

    def _read(self, name):
        try:
            with open(os.path.join(self.dir, name)) as f:
                return float(f.read().strip())
        except (OSError, ValueError):
            return None

    def _run(self):
        while not self._stop.is_set():
            f, p = self._read("freq1_input"), self._read("power1_input")
            if f:
                self.sclk.append(f * 1e-6)
            if p:
                self.power.append(p * 1e-6)
            self._stop.wait(self.period)

    def start(self):
        if self._thread:
            self._thread.start()

    def stop(self):
        if self._thread:
            self._stop.set()
            self._thread.join(timeout=1.0)

    def summary(self):
        if not self.sclk:
            return None
        cap = self._read("power1_cap")
        out = {"sclk_mhz_mean": round(sum(self.sclk) / len(self.sclk), 1), "sclk_mhz_min": round(min(self.sclk), 1),
               "sclk_mhz_max": round(max(self.sclk), 1), "peak_sclk_mhz": PEAK_SCLK_MHZ, "samples": len(self.sclk),
               "source": "hwmon freq1_input / power1_input of rank 0's GPU every %d ms over up to 12 further steps of the "
                         "same form right after the timed region (not timed)" % int(self.period * 1e3)}
        if self.power:
            out["power_w_mean"] = round(sum(self.power) / len(self.power), 1)
        if cap:
            out["power_cap_w"] = round(cap * 1e-6, 1)
        return out


def pin_rank(local):
    """Pin this rank's threads to the CPUs next to its GPU BEFORE anything touches the GPU; -> the `affinity` block of
    the JSON line, or None.  spawn_ranks hands the set over in SF_RANK_CPUS; under torch.distributed.run (the driver's
    N > 1 form), which pins nothing, the rank takes the set spawn_ranks would have given its LOCAL_RANK (sysfs only).
    SF_BENCH_PIN=0 switches the pinning off."""
    if os.environ.get("SF_BENCH_PIN", "1") == "0":
        return None
    if "SF_RANK_CPUS" not in os.environ and "RANK" in os.environ and int(os.environ.get("LOCAL_WORLD_SIZE", "1")) > 1:
        try:
            node, cpus = rank_cpu_sets(int(os.environ["LOCAL_WORLD_SIZE"]))[local]
            os.environ["SF_RANK_CPUS"] = ",".join(str(c) for c in cpus)
            os.environ["SF_RANK_NUMA"] = str(node)
        except (OSError, ValueError, IndexError):
            return None
    if not os.environ.get("SF_RANK_CPUS"):
        return None
    try:
        cpus = sorted(int(c) for c in os.environ["SF_RANK_CPUS"].split(",") if c)
        os.sched_setaffinity(0, cpus)
        return {"numa_node": int(os.environ.get("SF_RANK_NUMA", "-1")), "cpus": len(cpus), "first_cpu": cpus[0],
                "last_cpu": cpus[-1]}
    except (OSError, ValueError, IndexError):
        return None


def spawn_selftest(rank, world):
    """--spawn-selftest: the launcher's contract without a GPU (tests/test_distributed_cpu.py)."""
    import torch.distributed as dist
    if os.environ.get("SF_SELFTEST_FAIL_RANK") == str(rank):
        raise SystemExit(3)
    affinity = pin_rank(int(os.environ.get("LOCAL_RANK", "0")))
    if "RANK" in os.environ:
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    ones = torch.ones(1)
    pinned = torch.tensor([1.0 if affinity and len(os.sched_getaffinity(0)) == affinity["cpus"] else 0.0])
    if dist.is_initialized():
        dist.all_reduce(ones)
        dist.all_reduce(pinned)
    if rank == 0:
        print("[bench] selftest: %d of %d ranks pinned themselves" % (int(pinned.item()), world), file=sys.stderr)
        print(json.dumps({"selftest": True, "n_gpus": world, "n_ranks_seen": int(ones.item())}))
    if dist.is_initialized():
        dist.destroy_process_group()


def settle(measure, device, cap=40, group=4, tol=0.02, min_ms=0.0):
    """Run `measure(group)` -> (ms per step, host issue ms per step) until two successive groups take the same time
    within tol (at most `cap` steps) AND at least `min_ms` of stepping have gone by (then up to cap + min_ms worth of
    steps); -> ((ms, issue ms), steps run).  With a process group of more than one rank every rank must run the SAME
    number of steps (each step holds collectives): the decisions are taken on the slowest rank's times, which all ranks
    see identically after one MAX all-reduce per group.
    min_ms (the first search of a run only): as the FIRST GPU process of a fresh box the first ~3 s of steps carry
    one-off host stalls of 50-100 ms (library pages and runtime pools touched for the first time; round 3: tools/
    cold_start.py) — two groups of four steps agree long before those are over, and ONE such stall inside 20 timed
    steps is + 3.6 ms per step (round 6, driver command on fresh boxes: 55.2 / 55.3 / 57.3 ms where the same box's
    second process and the run's own steady-state search read 51.3-51.6)."""
    prev, n, spent, best, limit = None, 0, 0.0, None, cap
    while True:
        cur = tuple(measure(group))
        n += group
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor(cur, dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            cur = tuple(t.tolist())
        if prev is None and min_ms > 0:
            limit = cap + int(min_ms / max(cur[0], 1e-3))  # never more than cap + min_ms worth of steps
        spent += cur[0] * group
        steady = prev is not None and abs(cur[0] - prev[0]) <= tol * min(cur[0], prev[0])
        if steady:
            cand = min(cur, prev)
            best = cand if best is None or cand < best else best
        if (steady and spent >= min_ms) or n >= limit:
            return (best if best is not None else cur), n
        prev = cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    # 30 warm-up steps (2 s) by default: as the FIRST GPU process on a fresh box the first ~2-3 s of steps carry
    # one-off host stalls (runtime pools growing, rarely used code objects loading, allocator growth: tools/
    # cold_start.py shows 90-100 ms groups among 68.7 ms ones) — measured as first process: 71.7 / 70.2 ms per step with
    # 8 warm-up steps, 68.2 with 60; every later process on the same box: 67.9-68.3 with 8
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--workload", default="dual", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="clips per GPU (default: the workload's)")
    ap.add_argument("--mode", default="train", choices=["train", "eval"])
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--graph-train", action="store_true", help="(train) capture the whole step into one hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-overlap-allreduce", action="store_true",
                    help="(train) ONE all-reduce after the backward instead of chunks issued as the stages' gradients land")
    ap.add_argument("--spawn-selftest", action="store_true",
                    help="CPU-only check of the launcher logic: ranks join a gloo group, all-reduce ones, rank 0 prints")
    ap.add_argument("--no-extras", action="store_true",
                    help="profiling aid (with --full): skip the clock probe, the secondary eval-forward measurement and "
                         "the HIP-event roofline trace so that a rocprofv3 --stats run contains exactly warmup+steps "
                         "identical steps")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline figure: clocks, eval forward, roofline trace, CPU baseline with the "
                         "oracle parity fields and gate, gradient hash (--no-extras / --no-cpu-baseline narrow it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs to DIR/<name>.npy (float32, at most 64 MB)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.spawn_selftest:
        if "RANK" not in os.environ and args.gpus > 1:
            raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
        return spawn_selftest(rank, world)
    if (args.gpus > 1 or os.environ.get("SF_BENCH_FORCE_SPAWN") == "1") and "RANK" not in os.environ:
        # called directly: become the launcher.  Nothing in this process has touched the GPU yet (no HIP call, no
        # torch.cuda.is_available()), and it never will: the children do the work
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    if args.gpus != world:
        raise SystemExit("--gpus %d but the launcher started %d ranks" % (args.gpus, world))
    affinity = pin_rank(local)
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback for the hot path)"
    # TEST-ONLY overrides (tests/test_multigpu_gpu.py runs the whole N = 2 path of this file on a 1-GPU box):
    # SF_BENCH_ONE_DEVICE=1 puts every rank on device 0, SF_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on
    # one device).  Both are reported in the JSON line (config.parallelism) so such a line cannot pass for a scaling run.
    one_device = os.environ.get("SF_BENCH_ONE_DEVICE") == "1"
    backend = os.environ.get("SF_BENCH_BACKEND", "nccl")
    if one_device:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import torch.distributed as dist
    if world > 1 or "RANK" in os.environ:  # one process per GPU (torch.distributed.run, or spawn_ranks above)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)  # "nccl" = RCCL over xGMI
    # the ranks RCCL really connected: an all-reduce of ones
    ones = torch.ones(1, device=device)
    if dist.is_initialized():
        dist.all_reduce(ones)
    n_ranks_seen = int(ones.item())

    import sfhip
    from slowfast.utils.distributed import FlatGradients, max_over_ranks
    cfg, model, batch, desc = build(args.workload, device)
    batch = args.batch or batch
    clips = synthetic_clips(cfg, batch, device, 100 + rank)  # a different shard of clips per rank
    labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (batch,), device=device,
                           generator=torch.Generator(device=device).manual_seed(7 + rank))
    train = args.mode == "train"
    side = torch.cuda.Stream(priority=int(os.environ.get("SF_PRIO_MAIN", "0")))
    # the seeded state (host copy), restored in place right before the timed steps: what they compute then does not
    # depend on how many warm-up / steady-state steps ran before them
    start_state = {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()} if train else None

    if train:
        step, flat, opt = make_train_step(model, clips, labels, overlap_allreduce=not args.no_overlap_allreduce)
    else:
        def step():
            with torch.no_grad():
                return model([clips[0], clips[1]])

    # ---- warm-up (also builds the packed-weight / folded-BN caches): the W steps asked for, then on to a STEADY state
    #      whatever W was — groups of 4 steps until two successive groups agree within 2 % (at most 40 more steps).  As
    #      the first GPU process of a fresh box the first 2-3 s of steps carry one-off host stalls (runtime pools
    #      growing, code objects loading, allocator growth: tools/cold_start.py), and round 4's driver run (--warmup 5)
    #      decided the launch form on exactly those steps.  Nothing here is timed for the result.
    with torch.cuda.stream(side):
        for _ in range(max(args.warmup, 1)):
            out = step()
    torch.cuda.synchronize()

    def ms_per(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            for _ in range(n):
                fn()
        t_issue = time.perf_counter() - t0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, t_issue / n * 1e3

    (eager_ms, issue_ms), settle_steps = settle(lambda n: ms_per(step, n), device,
                                                min_ms=float(os.environ.get("SF_BENCH_SETTLE_MS", "3000")))
    launch_probe = {"steady_state_steps": settle_steps, "eager_ms": round(eager_ms, 3),
                    "host_issue_ms": round(issue_ms, 3)}
    graph = None
    graph_note = None
    graph_logits = None  # (train) the captured step's static logits

    # With a process group up, RCCL's watchdog thread polls its events at any time: under the default (global)
    # capture mode such a call from ANOTHER thread aborts the process ("operation not permitted when stream is
    # capturing"); thread-local mode restricts the check to the capturing thread's own calls.
    capture_mode = "thread_local" if dist.is_initialized() else "global"

    def capture():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode=capture_mode):
            o = step()
        g.replay()
        torch.cuda.synchronize()
        return g, o

    want_graph = (not train and not args.no_graph) or (train and args.graph_train)
    auto = False
    if train and not args.graph_train and not args.no_graph and world == 1 and not dist.is_initialized():
        # Launch-bound training steps (cfg #1: ~1500 launches of a 0.007 GMAC model): when the Python thread needs as
        # long to ISSUE a warm step as the GPU needs to run it, the step is also captured into one hipGraph, BOTH forms
        # are timed warm, and the faster one is what the timed region runs.  For cfg #2 / #3 the warm host is 1.4-2x
        # ahead and nothing is captured.  Not with a process group up: the step then holds RCCL collectives on a comm
        # stream, which stay eager.
        if issue_ms > 0.85 * eager_ms:
            want_graph = auto = True
    if want_graph:
        # eval forward: one hipGraph.  The train step (forward, backward with the tape's streams as graph branches,
        # SGD) also captures (the capture runs right after an optimizer step, so every conv's weight re-packing is part
        # of the graph).
        try:
            graph, out = capture()
            graph_logits = step.logits if train else None
            if auto:
                (graph_ms, _), _n = settle(lambda n: ms_per(graph.replay, n), device, cap=24)
                launch_probe["graph_ms"] = round(graph_ms, 3)
                # torch.cuda.graph() emptied the allocator's cache before capturing: the first eager steps after it
                # re-allocate every block of the step (measured: 82 ms per step over the next 20 instead of 59) — the
                # eager form is warmed up again and RE-TIMED before the two warm figures are compared
                (eager_ms, issue_ms), _n = settle(lambda n: ms_per(step, n), device, cap=24)
                launch_probe["eager_ms_after_capture"] = round(eager_ms, 3)
                launch_probe["host_issue_ms_after_capture"] = round(issue_ms, 3)
                if graph_ms >= min(eager_ms, launch_probe["eager_ms"]):
                    graph = graph_logits = None  # drops the graph and its private memory pool
                    graph_note = "eager (host-bound, but the warm hipGraph replay was not faster)"
                    settle(lambda n: ms_per(step, n), device, cap=12)
                launch_probe["timed"] = "eager" if graph is None else "hipGraph replay"
        except Exception as e:  # noqa: BLE001 — fall back to eager launches and say so in the JSON line
            graph, graph_note = None, "hipGraph capture failed (%s: %s); eager launches" % (type(e).__name__, str(e)[:120])
            graph_logits = None
            torch.cuda.synchronize()
            settle(lambda n: ms_per(step, n), device, cap=12)
    if graph is None:
        with torch.cuda.stream(side):
            out = step()  # the tensor the finiteness check reads belongs to the form that is timed
        torch.cuda.synchronize()
    else:
        graph.replay()  # `out` is the capture's static output: rewritten by every replay
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "non-finite model output"
    launch_probe.setdefault("timed", "eager" if graph is None else "hipGraph replay")

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    # ---- the timed steps start from the seeded state: parameters and buffers as build() left them, zero momentum
    #      (the SGD update of a zero buffer is the first step's), a seeded dropout generator.  In place: a captured graph
    #      reads the same addresses.
    if train:
        from slowfast.models import engine as _eng
        with torch.no_grad():
            for k, v in model.state_dict().items():
                v.copy_(start_state[k])
            for st in opt.state.values():
                if st.get("momentum_buffer") is not None:
                    st["momentum_buffer"].zero_()
        torch.manual_seed(1000 + rank)
        _eng.parameters_changed()
        torch.cuda.synchronize()

    # ---- host-side hygiene before timing: a full (generation-2) collection of the Python garbage collector walks
    # every tracked object of the process (modules, parameters, caches: ~10^6) and stalls the launch thread for ~80 ms
    # about every 20 steps — longer than the launch queue is deep, so the GPU idles (tools/cold_start.py: groups of 4
    # steps at 68.6 ms with one of 88 ms every fifth group).  Collect once, then FREEZE what exists (gc.freeze moves it
    # to the permanent generation): the collector stays on, but what it walks from now on is one step's garbage.
    import gc
    gc.collect()
    gc.freeze()

    # ---- timed region: exactly K steps
    barrier()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for _ in range(args.steps):
            if graph is not None:
                graph.replay()   # (the epoch bump of engine.replay is hoisted: parameters_changed() right after the loop)
            else:
                out = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if graph is not None and train:
        from slowfast.models import engine as _eng
        _eng.parameters_changed()  # replayed optimizer kernels moved the parameters: every eager cache is stale
    barrier()
    elapsed = max_over_ranks(elapsed, device)
    # the LAST timed step's own result (eager: the tensor it returned; replay: the capture's static output, which every
    # replay rewrites): train = the loss, eval = the probabilities
    assert bool(torch.isfinite(out).all()), "non-finite result in the timed region"
    last_loss = float(out.detach()) if train else None
    if args.dump_outputs and rank == 0:  # before anything below moves the parameters
        dump_outputs(args.dump_outputs, train_outputs(model, out, graph_logits if graph is not None else step.logits)
                     if train else {"probabilities": out})
    extras = args.full and not args.no_extras  # (plain runs and --no-extras: exactly W + steady-state + K steps)
    # ---- clock probe: the same steps once more, NOT timed, with the sampler thread reading the hwmon files (inside the
    #      timed region the reads cost nothing on most boxes and 3.6 ms per step on one with a slow host: the driver's
    #      sysfs handlers and the launch thread meet somewhere).  Every rank runs the steps (they carry the collective).
    clock_sampler = None
    if extras and os.environ.get("SF_BENCH_CLOCKS", "1") != "0":
        clock_sampler = ClockSampler(gpu_hwmon_dir(local) if rank == 0 else None,
                                     period=float(os.environ.get("SF_BENCH_CLOCKS_PERIOD", "0.05")))
        clock_sampler.start()
        with torch.cuda.stream(side):
            for _ in range(min(args.steps, 12)):
                if graph is not None:
                    graph.replay()
                else:
                    out_probe = step()
        torch.cuda.synchronize()
        clock_sampler.stop()
        if graph is not None and train:
            from slowfast.models import engine as _eng
            _eng.parameters_changed()
        barrier()

    # ---- secondary: eval-mode forward (inference) clips/s of the same model, hipGraph replay
    eval_fwd = None
    if train and extras:
        model.eval()

        def estep():
            with torch.no_grad():
                return model([clips[0], clips[1]])

        with torch.cuda.stream(side):
            estep()
        torch.cuda.synchronize()
        eg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(eg, stream=side, capture_error_mode=capture_mode):
            estep()
        eg.replay()
        barrier()
        t1 = time.perf_counter()
        with torch.cuda.stream(side):
            for _ in range(args.steps):
                eg.replay()
        torch.cuda.synchronize()
        et = max_over_ranks(time.perf_counter() - t1, device)
        barrier()
        eval_fwd = {"value": round(batch * world * args.steps / et, 3), "unit": "clips/s",
                    "ms_per_step": round(et / args.steps * 1e3, 3), "launch": "hipGraph replay"}
        model.train()

    # ---- dominant-kernel trace: HIP events around every attention / dense-conv / depthwise-conv C-ABI call over a few
    #      eager steps on ONE stream (the two-stream schedule is switched off for these steps, so an event pair times its
    #      kernel(s) and not a neighbour running beside them).  The (kernel, shape) with the largest total time per step
    #      is the roofline object: algorithmic FLOPs or bytes of one launch / its average duration.
    roofline = None
    family_ms = None
    launch_bound = None
    if extras:  # every rank runs the traced steps (they carry the step's collective); rank 0 reports
        from slowfast.models import engine as _engine
        sfhip.EVENT_TRACE = []
        nsteps = min(args.steps, 3)
        saved_overlap, _engine.OVERLAP_PATHS = _engine.OVERLAP_PATHS, False
        try:
            with torch.cuda.stream(side):
                step()  # one un-traced step in the serial schedule first (allocator pools of the single stream)
                sfhip.EVENT_TRACE = []
                calls0 = sfhip.CALLS
                for _ in range(nsteps):
                    step()
                abi_calls_per_step = (sfhip.CALLS - calls0) / float(nsteps)
            torch.cuda.synchronize()
        finally:
            _engine.OVERLAP_PATHS = saved_overlap
        trace, sfhip.EVENT_TRACE = sfhip.EVENT_TRACE, None
        if rank == 0 and trace:
            per = {}
            for tag, e0, e1 in trace:
                per.setdefault(tag, []).append(e0.elapsed_time(e1) * 1e-3)
            tot = {tag: sum(v) for tag, v in per.items()}
            fam = {}
            for tag, v in tot.items():
                f = "attention" if tag[0].startswith("attn") else tag[0]
                fam[f] = fam.get(f, 0.0) + v
            family_ms = {f: round(v / nsteps * 1e3, 3) for f, v in sorted(fam.items(), key=lambda kv: -kv[1])}
            # launch-bound models (cfg #1): what the step would take if every traced launch ran at its own floor —
            # max(algorithmic FLOPs / MFMA peak, output (conv) or in+out (depthwise) bytes / 8 TB/s) — beside the number
            # of C-ABI calls one step issues; the distance between that sum and the measured step is launch latency and
            # dependency stalls, not kernel quality
            floors = 0.0
            for t_, v_ in per.items():
                if t_[0] == "conv":
                    f_ = max(2.0 * t_[1] * t_[2] * t_[3] / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4.0 * t_[1] * t_[3] / 8e12)
                elif t_[0] == "dwconv":
                    f_ = t_[1] / 8e12
                elif t_[0].startswith("attn"):
                    np_ = {"attn": 2, "attn_bwd_dkv": 3, "attn_bwd_dq": 2, "attn_bwd_fused": 5}.get(t_[0], 2)
                    f_ = np_ * 2.0 * t_[1] * t_[2] * t_[2] * t_[3] / (PEAK_FP32_MFMA_TFLOPS * 1e12)
                else:
                    f_ = 0.0
                floors += f_ * len(v_)
            launch_bound = {"abi_calls_per_step": round(abi_calls_per_step, 1),
                            "traced_launches_per_step": round(len(trace) / float(nsteps), 1),
                            "traced_kernel_ms_per_step": round(sum(tot.values()) / nsteps * 1e3, 3),
                            "sum_of_kernel_floors_ms": round(floors / nsteps * 1e3, 4),
                            "note": "C-ABI calls (conv / depthwise / attention / BN / elementwise; torch's own loss and "
                                    "optimizer kernels not counted) of one step; floors: per traced conv / depthwise / "
                                    "attention launch max(FLOP / f32 MFMA peak, bytes / 8 TB/s)"}
            tag = max(tot, key=tot.get)
            top_family = "attention" if tag[0].startswith("attn") else tag[0]
            dur = float(np.mean(per[tag]))
            if top_family == "attention":
                kind, b, n, c = tag
                # algorithmic FLOPs, one product = 2*N^2*C FLOP per clip.  Forward: QK^T + PV = 2.
                # Backward: 5 products in total (S recompute, dP, dV, dK, dQ); the two-kernel, atomic-free split
                # re-derives S and dP in both kernels (7 executed), so each kernel is credited only its share of the 5:
                # dK/dV kernel = dV + dK + half of (S, dP) = 3, dQ kernel = dQ + the other half = 2.
                # The single-sweep backward (attn_bwd_fused: dK/dV/dQ kernel + the dQ plane reduction, timed together)
                # executes exactly the 5 algorithmic products.
                nprod = {"attn": 2, "attn_bwd_dkv": 3, "attn_bwd_dq": 2, "attn_bwd_fused": 5}[kind]
                executed = {"attn": 2, "attn_bwd_dkv": 4, "attn_bwd_dq": 3, "attn_bwd_fused": 5}[kind]
                flops = nprod * 2.0 * b * n * n * c
                ach = flops / dur / 1e12
                # 17 <= d <= 32: every fp32 product runs as six bf16 MFMAs on three-way split operands (attn_bx.h);
                # the pipe this kernel is bound by is then the bf16 one, and its ceiling in ALGORITHMIC fp32 FLOP/s is
                # the dense bf16 peak / 6
                split6 = sfhip.lib().sf_attn_products_per_fp32(c) == 6 and kind in ("attn", "attn_bwd_fused")
                kname = {"attn": "attn_fwd_kernel (flash SpatialAttention forward)",
                         "attn_bwd_dkv": "attn_bwd_dkv_kernel (flash SpatialAttention backward, dK/dV)",
                         "attn_bwd_dq": "attn_bwd_dq_kernel (flash SpatialAttention backward, dQ)",
                         "attn_bwd_fused": "attn_bwd_fused_kernel + attn_dq_reduce_kernel (flash SpatialAttention "
                                           "backward, dQ/dK/dV in one sweep)"}[kind]
                traffic, traffic_src = None, None  # HBM bytes per launch: rocprofv3 PMC passes cannot run inside bench.py
                try:
                    tfile = next(f for f in ("r05_attention_hbm_traffic.json", "r04_attention_hbm_traffic.json",
                                             "r03b_attention_hbm_traffic.json", "r03_attention_hbm_traffic.json",
                                             "r02b_attention_hbm_traffic.json")
                                 if os.path.exists(os.path.join(ROOT, "profiles", f)))
                    tj = json.load(open(os.path.join(ROOT, "profiles", tfile)))["kernels"]
                    if kind == "attn_bwd_fused" and c == 32 and n == 25088 and b == 8:
                        # the sweep kernel + its three reductions (dQ partials: tiled kernel; dK parts, dV parts)
                        g = -(-(b * n * 8) // 256) * 256
                        sweep = [v for k, v in tj.items() if k.startswith(
                            "attn_bwd_bx_kernel" if split6 else "attn_bwd_fused_kernel<32, 4>")]
                        if split6:  # + the two launches that write the bf16 planes of Q and gamma dz
                            sweep[0] = dict(sweep[0], hbm_bytes_per_launch=sweep[0]["hbm_bytes_per_launch"] + 2 * next(
                                v for k, v in tj.items() if k.startswith("attn_bx_split_kernel"))["hbm_bytes_per_launch"])
                        traffic = (sweep[0]["hbm_bytes_per_launch"] + tj["attn_dq_reduce_tiled_kernel grid=%d" % g]["hbm_bytes_per_launch"]
                                   + 2 * tj["attn_dq_reduce_kernel grid=%d" % g]["hbm_bytes_per_launch"])
                        traffic_src = "profiles/%s (rocprofv3 PMC passes FETCH_SIZE / WRITE_SIZE of the same kernels, " \
                                      "tools/attn_traffic.sh; not measured in this run)" % tfile
                except (OSError, KeyError, ValueError, IndexError, StopIteration):
                    traffic = None
                peak = PEAK_BF16_MFMA_TFLOPS / 6.0 if split6 else PEAK_FP32_MFMA_TFLOPS
                if split6:
                    kname = {"attn": "sf_attn_bx_split x2 + attn_fwd_bx_kernel (flash SpatialAttention forward",
                             "attn_bwd_fused": "sf_attn_bx_split x2 + attn_bwd_bx_kernel + attn_dq_reduce kernels (flash "
                                               "SpatialAttention backward, dQ/dK/dV in one sweep"}[kind] + \
                        "; fp32 operands as three bf16 pieces, six v_mfma_f32_32x32x16_bf16 per fp32 product)"
                roofline = {"bound": "mfma", "kernel": "%s C=%d N=%d B=%d" % (kname, c, n, b),
                            "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                            "frac": round(ach / peak, 4), "avg_launch_ms": round(dur * 1e3, 4),
                            "launches_timed": len(per[tag]), "traffic": traffic, "traffic_source": traffic_src,
                            "executed_mfma_tflops": round(ach * (6.0 if split6 else executed / nprod), 2)}
                if split6:
                    roofline["frac_of_f32_mfma_peak"] = round(ach / PEAK_FP32_MFMA_TFLOPS, 4)  # the round-2 / 3a basis
                    roofline["peak_basis"] = ("algorithmic fp32 FLOP/s against the dense bf16 MFMA peak (%.0f TFLOP/s) / 6 "
                                              "products per fp32 product; executed_mfma_tflops is the bf16 rate; the "
                                              "f32-input MFMA peak this path replaces is %.1f TFLOP/s" % (
                                                  PEAK_BF16_MFMA_TFLOPS, PEAK_FP32_MFMA_TFLOPS))
            elif top_family == "conv":
                _, m, k, n = tag
                ach = 2.0 * m * k * n / dur / 1e12
                # the conv family as a whole: algorithmic FLOPs of every traced launch / their summed durations
                fl = sum(2.0 * t[1] * t[2] * t[3] * len(v) for t, v in per.items() if t[0] == "conv")
                agg = fl / fam["conv"] / 1e12
                roofline = {"bound": "mfma", "kernel": "conv_wave_kernel / conv_wgrad_wave_kernel (dense 3-D conv as "
                            "implicit GEMM; forward, data- and weight-gradient launches of the shape positions=%d, "
                            "taps*Cin=%d, Cout=%d)" % (m, k, n),
                            "achieved": round(ach, 4), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                            "frac": round(ach / PEAK_FP32_MFMA_TFLOPS, 6), "avg_launch_ms": round(dur * 1e3, 4),
                            "launches_timed": len(per[tag]), "traffic": None,
                            "conv_family": {"achieved": round(agg, 2), "frac": round(agg / PEAK_FP32_MFMA_TFLOPS, 4),
                                            "note": "algorithmic FLOPs of ALL dense-conv launches of a step / the sum of "
                                                    "their HIP-event durations (conv-arithmetic roofline, SURVEY 8d)"}}
            else:  # depthwise convs: HBM-bound
                by = sum(t[1] * len(v) for t, v in per.items() if t[0] == "dwconv")
                ach = by / fam["dwconv"] / 1e9
                roofline = {"bound": "hbm", "kernel": "dwconv_kernel (depthwise 3-D conv, GhostNet / ShuffleNetV2 paths)",
                            "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4),
                            "launches_timed": sum(len(v) for t, v in per.items() if t[0] == "dwconv"), "traffic": None}
            # the HBM-bound depthwise family beside the dominant one (cfg #5's "bandwidth-bound stress")
            if "dwconv" in fam and roofline is not None and top_family != "dwconv":
                by = sum(t[1] * len(v) for t, v in per.items() if t[0] == "dwconv")
                roofline["dwconv_hbm"] = {"achieved": round(by / fam["dwconv"] / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                                          "frac": round(by / fam["dwconv"] / 1e9 / 8000.0, 4),
                                          "ms_per_step": family_ms["dwconv"]}

    def hip_train_step(xs, label):  # one HIP training step on the oracle's clip, dropout off (the oracle has none)
        drops = [(m, m.p) for m in model.modules() if isinstance(m, torch.nn.Dropout)]
        for m, _ in drops:
            m.p = 0.0
        try:
            with torch.cuda.stream(side):
                flat.zero()
                logits = model(xs)
                loss = torch.nn.functional.cross_entropy(logits, label)
                loss.backward()
            torch.cuda.synchronize()
        finally:
            for m, p_ in drops:
                m.p = p_
        return float(loss), logits.detach(), {k: v.grad.detach().clone() for k, v in model.named_parameters()
                                              if v.grad is not None}

    # ---- parity on the TRAINED state (secondary fields *_after_steps): the HIP path against the oracle on the parameters,
    #      BN buffers and momentum the timed SGD steps on random labels left — BEFORE anything re-fills them (the
    #      gradient-hash step below starts from the seeded fill), so that a regression of the kernels' accuracy at the
    #      weights the benchmark actually reached cannot hide behind the re-fill
    after = None
    if args.full and rank == 0 and world == 1 and train and not args.no_cpu_baseline:
        _, after = cpu_baseline(args.workload, cfg, model, train, device, hip_train_step, parity_only=True)

    # ---- the gradient buffer as ONE integer, on a canonical state: seeded parameters / BN buffers, seeded generator
    #      (dropout), one more step.  Every kernel and RCCL's reduction order are deterministic, so the chunked and the
    #      single-collective schedule must agree on it bit for bit (tests/test_multigpu_gpu.py) — the number of steps a
    #      run took to reach its steady state must not enter.  Every rank runs the step (it carries the collective).
    ghash = None
    if train and args.full:
        from paramgen import fill_state_dict
        with torch.no_grad():
            fill_state_dict(model.state_dict(), PARAM_SEED)
        torch.manual_seed(20250 + rank)
        with torch.cuda.stream(side):
            step()
        torch.cuda.synchronize()
        ghash = int(flat.flat.view(torch.int32).to(torch.int64).sum().item()) & 0xffffffffffff
    # every rank's hash and the number of steps its steady-state search ran (both must agree across ranks: the reduced
    # gradient is one buffer, and settle() decides on the MAX over ranks, so no rank may leave its loop alone)
    per_rank = None
    if args.full and dist.is_initialized() and world > 1:
        mine = torch.tensor([ghash if ghash is not None else -1, launch_probe["steady_state_steps"]],
                            dtype=torch.int64, device=device)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = {"grad_hash": [int(t[0]) for t in allr], "steady_state_steps": [int(t[1]) for t in allr]}

    if rank == 0:
        clips_total = batch * world * args.steps
        res = {
            "metric": "clips/sec (8x8 224^2 SlowFast-R50+CMDA, %s)" % ("train step fwd+bwd+allreduce+SGD" if train
                                                                          else "eval forward")
            if args.workload == "dual" else "clips/sec (%s, %s)" % (args.workload, args.mode),
            "value": round(clips_total / elapsed, 3), "unit": "clips/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": desc,
                       "mode": "train step: train-mode forward + CE + backward + 1 flat-gradient all-reduce + SGD (momentum 0.9, weight decay 1e-4; torch.optim.SGD%s)" % (", fused" if getattr(opt, "defaults", {}).get("fused") else "")
                       if train else "eval forward (inference)",
                       "clips_per_gpu": batch, "global_batch": batch * world, "layout": "NCTHW in, NDHWC inside",
                       "arithmetic": "fp32 tensors, fp32 accumulation everywhere; short-reduction convs and d = 128 "
                                     "attention on v_mfma_f32_*_f32; the long-reduction convs (forward, data and weight "
                                     "gradient of the 1x3x3 / 3x1x1 layers over >= 128 channels) and the attention "
                                     "products of head widths 17..64 and 8 as exact three-way bf16 splits, six "
                                     "v_mfma_f32_32x32x16_bf16 per fp32 product (fp32-level results: DESIGN 6a-4, 6a-5)"
                       if sfhip.lib().sf_attn_products_per_fp32(32) == 6 else "fp32 (v_mfma_f32_*_f32)",
                       "launch": (graph_note or "eager") if graph is None else (
                           "hipGraph replay" if not auto else
                           "hipGraph replay (the warm eager step is host-bound and the warm replay is faster)"),
                       "launch_probe": launch_probe,
                       "parallelism": "dp%d (clip-sharded replicas; %s)%s" % (
                           world, "one RCCL all-reduce of the flat fp32 gradient per step" if train
                           else "no data-path collective in forward",
                           "" if backend == "nccl" and not one_device else
                           " TEST CONFIGURATION: backend %s, all ranks on one device = %s - not a scaling measurement" % (
                               backend, one_device))},
        }
        res["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated(device) / 1e9, 2)  # of 288 GB
        # whole-step arithmetic roofline (algorithmic FLOPs per clip: convs x3 for fwd + dgrad + wgrad,
        # flash attention x3.5; fwd only in eval mode) against the dense-f32 MFMA peak of all GPUs in the job
        # cfg #5: conv 5.53 + attention 89.04 GMAC per clip forward -> 2 (3 x 5.53 + 3.5 x 89.04) GFLOP
        per_clip = {"dual": (211.3e9, 690.0e9), "slowfast": (100.6e9, 302.0e9),
                    "ghostnet": (189.1e9, 656.5e9)}.get(args.workload)
        if per_clip is not None:
            flop = per_clip[1 if train else 0] * clips_total
            ach = flop / elapsed / 1e12
            res["step_roofline"] = {"algorithmic_gflop_per_clip": per_clip[1 if train else 0] / 1e9,
                                    "achieved_tflops": round(ach, 2), "peak_tflops": PEAK_FP32_MFMA_TFLOPS * world,
                                    "frac": round(ach / (PEAK_FP32_MFMA_TFLOPS * world), 4)}
        clocks = clock_sampler.summary() if clock_sampler is not None else None
        if clocks is not None:
            res["clocks"] = clocks
            if "step_roofline" in res:  # the same fraction against the ceiling at the clock the part actually held
                res["step_roofline"]["frac_at_sustained_clock"] = round(
                    res["step_roofline"]["frac"] * PEAK_SCLK_MHZ / clocks["sclk_mhz_mean"], 4)
        if eval_fwd is not None:
            res["eval_forward"] = eval_fwd
        if roofline is not None:
            roofline["trace_schedule"] = "one stream (two-stream overlap off for the traced steps)"
            res["roofline"] = roofline
            res["kernel_family_ms_per_step"] = family_ms
        if launch_bound is not None:
            launch_bound["step_ms"] = res["ms_per_step"]
            launch_bound["host_issue_ms"] = launch_probe.get("host_issue_ms")
            launch_bound["launch_bound"] = bool(launch_probe.get("host_issue_ms", 0.0) > 0.85 * launch_probe.get("eager_ms", 1e9))
            res["launch_bound"] = launch_bound
        res["n_ranks_seen"] = n_ranks_seen
        if last_loss is not None:
            res["last_timed_step_loss"] = round(last_loss, 6)
        if affinity is not None:
            res["rank0_cpu_affinity"] = affinity
        if train:
            res["allreduce"] = {"chunks_per_step": flat.chunks_last_step,
                                "schedule": "one collective after the backward" if args.no_overlap_allreduce else
                                "flat fp32 gradient in chunks [s5+head | s4+s4_fuse | rest] on a comm stream, each issued "
                                "when its stages' backward is done, joined before the optimizer step",
                                "bytes": int(flat.flat.numel() * 4)}
            if ghash is not None:
                res["allreduce"]["grad_hash"] = ghash
            if per_rank is not None:
                res["allreduce"]["grad_hash_all_ranks"] = per_rank["grad_hash"]
                res["config"]["launch_probe"]["steady_state_steps_all_ranks"] = per_rank["steady_state_steps"]
        if args.full and world == 1 and not args.no_cpu_baseline:
            # parity on the SEEDED parameters (the state tests/test_fullsize_gpu.py bounds): the timed SGD steps on random
            # labels moved the weights, and after ~55 steps of them the same comparison read 5x larger gradient errors
            # (round 3: median 1.4e-3 against 2.6e-4) — weights, BN buffers and momentum-free: re-filled in place
            # ... and the same comparison on the TRAINED state first, as secondary fields (*_after_steps): a regression of
            # the kernels' accuracy at the weights the benchmark actually reached must not hide behind the re-fill
            from paramgen import fill_state_dict
            with torch.no_grad():
                fill_state_dict(model.state_dict(), PARAM_SEED)
            res["cpu_baseline"], parity = cpu_baseline(args.workload, cfg, model, train, device,
                                                       hip_train_step if train else None)
            # second half of BASELINE.json's metric: the HIP path against the oracle on the same full-size clip (batch 1).
            # fwd_max_rel_err: max|delta| / max|ref| over the eval output probabilities; fwd_logits_max_rel_err: the
            # same over the train-mode pre-activation logits (probabilities hide errors); bwd_*: relative
            # L2 error of every parameter's gradient of the training step (north_star tolerance: 1e-3 on the forward)
            for k, v in parity.items():
                res[k] = float("%.3e" % v) if isinstance(v, float) else v
            for k in ("fwd_logits_max_rel_err", "bwd_median_rel_err", "bwd_max_rel_err", "bwd_worst_param",
                      "bwd_median_rel_err_vs_fp64", "bwd_max_rel_err_vs_fp64", "bwd_worst_param_vs_fp64",
                      "oracle_fp32_vs_fp64_bwd_median", "oracle_fp32_vs_fp64_bwd_max"):
                if after and k in after:
                    v = after[k]
                    res[k + "_after_steps"] = float("%.3e" % v) if isinstance(v, float) else v
            res["parity_note"] = "HIP vs oracle (CPU restatement of the reference), 1 clip of the benchmark shape, on the " \
                                 "seeded parameters (re-filled after the timed steps; *_after_steps = the same comparison on the " \
                                 "state the timed SGD steps on random labels left, before the re-fill); forward tolerance 1e-3; bwd_* = " \
                                 "per-parameter relative L2 of the train step's gradients, the oracle differentiating with " \
                                 "the HIP forward's ReLU masks / max-pool winners (tests/_masks.py); gradients that are zero " \
                                 "in exact arithmetic (tests/_zero_grads.py) are bounded absolutely: bwd_zero_class_*; " \
                                 "*_vs_fp64 = the HIP step against the SAME oracle run in fp64 (same masks), " \
                                 "oracle_fp32_vs_fp64_* = the fp32 oracle against it: the reference's own rounding noise, " \
                                 "which is what bwd_max_rel_err sits on; " \
                                 "8-clip parity: tests/test_fullsize_gpu.py (eval rows vs 8 oracle forwards, 3-clip train step)"
    # ---- the gate: the line is printed either way, but a run whose forward or whose typical gradient is outside
    #      north_star's 1e-3 exits non-zero (bwd_max_rel_err is reported, not gated: single ill-conditioned parameters —
    #      DESIGN "Parity" — sit at the tolerance on the oracle's own fp32-vs-fp64 error)
    gate = []
    if rank == 0 and args.full:
        gate = parity_gate(res)
        res["parity_gate"] = "pass" if not gate else "FAIL: " + "; ".join(gate)
    elif rank == 0:
        res["parity_gate"] = "not run (the oracle comparison runs with --full)"
    if dist.is_initialized():
        dist.destroy_process_group()
    if rank == 0:
        # the JSON line is the LAST line of stdout: RCCL's version banner sits in C stdio's buffer since the group was
        # created and would otherwise be flushed behind it at exit (stdout redirected to a file or a pipe)
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(json.dumps(res), flush=True)
    if gate:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
