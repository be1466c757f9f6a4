"""Precise-BN pass: replace the exponential running statistics by the plain average of per-batch statistics
over `num_iters` training-mode forwards with frozen weights.  The reference calls fvcore's
`update_bn_stats(model, loader, num_iters)` from `calculate_and_update_precise_bn` (tools/train_net.py:277-296,
vendored fvcore/nn/precise_bn.py); fvcore is not part of this image, so the two entry points live here under the
same names.  The forwards run the HIP path: momentum 1.0 makes `sf_bn_train_stats` write the batch statistics
straight into running_mean / running_var, which are then averaged on the device."""
import itertools

import torch
from torch import nn

BN_MODULE_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def get_bn_modules(model):
    """All BN layers that are in training mode (SubBatchNorm3d contributes its inner `bn` and `split_bn`)."""
    return [m for m in model.modules() if m.training and isinstance(m, BN_MODULE_TYPES)]


@torch.no_grad()
def update_bn_stats(model, data_loader, num_iters=200):
    """model: in training mode for the layers that need precise statistics; data_loader: iterable of model inputs.

    The averaging is ONE native call per iteration (`sf_avg_update`, mode 2) over a table of {accumulator view,
    running_mean / running_var} pairs of all layers — the accumulators are views of one allocation, the iteration
    count a word in device memory — instead of six small torch operations per layer.  Per element it is what those
    operations computed on the GPU, bit for bit: mean += (running - mean) / (k + 1), where torch's division by the host
    number k + 1 is a multiply by its float32 reciprocal.  At the end one `sf_avg_exchange` launch writes the
    accumulators into the running statistics (in place: the buffers keep their addresses)."""
    from slowfast.models import engine, weight_avg
    from slowfast.models.step_tail import carve_views
    layers = get_bn_modules(model)
    if not layers:
        return
    saved = [bn.momentum for bn in layers]
    for bn in layers:
        bn.momentum = 1.0
    stats = [t for bn in layers for t in (bn.running_mean, bn.running_var)]
    for t in stats:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("precise-BN pass: running statistics must be contiguous float32 tensors, got %s" % t.dtype)
    _, acc = carve_views([t.numel() for t in stats], stats[0].device)
    pairs = [(a, t, weight_avg.KIND_AVG) for a, t in zip(acc, stats)]
    table = weight_avg._PairTable("precise-BN pass")
    count = torch.zeros((), dtype=torch.int64, device=stats[0].device)
    ind = -1
    for ind, inputs in enumerate(itertools.islice(data_loader, num_iters)):
        model(inputs)
        weight_avg.avg_update(*table.args(pairs), weight_avg.MODE_RUNNING, count)
    if ind != num_iters - 1:
        raise AssertionError("precise-BN pass: the loader ran dry after %d of the %d batches asked for" % (ind + 1, num_iters))
    weight_avg.avg_exchange(*table.args(pairs), weight_avg.OP_TO_SOURCE)
    engine.parameters_changed()  # the running statistics moved behind torch's version counters
    for i, bn in enumerate(layers):
        bn.momentum = saved[i]
