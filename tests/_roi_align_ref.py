"""float64 torch restatement of detectron2's ROIAlign as ResNetRoIHead calls it (sampling_ratio 0 by default, aligned
or legacy), written from its published semantics:

  offset = 0.5 if aligned else 0;  start = coord * spatial_scale - offset;  roi = end - start (legacy: max(roi, 1));
  bin = roi / R;  grid = ceil(roi / R) per dimension (sampling_ratio 0);  count = max(gh * gw, 1);
  sample (iy, ix) of bin (ph, pw): y = start_h + ph * bin_h + (iy + 0.5) * bin_h / gh (x likewise);
  bilinear: y < -1 | y > H | x < -1 | x > W -> 0; negative coordinates clamp to 0; floor(y) >= H-1 -> both rows H-1;
  bin value = sum of the samples / count.

Every sample is enumerated literally into a [R*R, H*W] weight matrix per box, so the result is differentiable with
respect to the features through torch autograd.  Used by the CPU tests (pinned against analytic cases), the GPU tests
(the HIP kernels against it) and tests/golden/make_golden_detection.py (stands in for detectron2's compiled op when
the reference itself runs)."""
import math

import torch
import torch.nn as nn


def _axis(y, H):
    """(lo, hi, weight of hi) of one sample coordinate, or None when the sample contributes 0."""
    if y < -1.0 or y > H:
        return None
    y = max(y, 0.0)
    lo = int(y)
    if lo >= H - 1:
        return H - 1, H - 1, 0.0
    return lo, lo + 1, y - lo


def roi_weights(box, H, W, output_size, spatial_scale, sampling_ratio=0, aligned=True):
    """float64 [R*R, H*W] matrix M with bins = M @ map.view(H*W) for one box row (x1, y1, x2, y2)."""
    Rh, Rw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    x1, y1, x2, y2 = [float(v) for v in box]
    off = 0.5 if aligned else 0.0
    sw, sh = x1 * spatial_scale - off, y1 * spatial_scale - off
    rw, rh = x2 * spatial_scale - off - sw, y2 * spatial_scale - off - sh
    if not aligned:
        rw, rh = max(rw, 1.0), max(rh, 1.0)
    bh, bw = rh / Rh, rw / Rw
    gh = sampling_ratio if sampling_ratio > 0 else max(int(math.ceil(rh / Rh)), 0)
    gw = sampling_ratio if sampling_ratio > 0 else max(int(math.ceil(rw / Rw)), 0)
    count = max(gh * gw, 1)
    M = torch.zeros(Rh * Rw, H * W, dtype=torch.float64)
    for ph in range(Rh):
        for pw in range(Rw):
            row = M[ph * Rw + pw]
            for iy in range(gh):
                ay = _axis(sh + ph * bh + (iy + 0.5) * bh / gh, H)
                if ay is None:
                    continue
                for ix in range(gw):
                    ax = _axis(sw + pw * bw + (ix + 0.5) * bw / gw, W)
                    if ax is None:
                        continue
                    (ylo, yhi, ly), (xlo, xhi, lx) = ay, ax
                    hy, hx = 1.0 - ly, 1.0 - lx
                    row[ylo * W + xlo] += hy * hx / count
                    row[ylo * W + xhi] += hy * lx / count
                    row[yhi * W + xlo] += ly * hx / count
                    row[yhi * W + xhi] += ly * lx / count
    return M


def roi_align(input, rois, output_size, spatial_scale, sampling_ratio=0, aligned=True):
    """input [N, C, H, W], rois [K, 5] (batch_idx, x1, y1, x2, y2) -> [K, C, Rh, Rw] in float64 (autograd flows to
    input).  A box whose batch index does not truncate into [0, N) gives zeros."""
    Rh, Rw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    x = input.to(torch.float64)
    N, C, H, W = x.shape
    outs = []
    for r in rois.detach().to(torch.float64).cpu():
        b = float(r[0])
        if not (-1.0 < b < N):
            outs.append(torch.zeros(C, Rh, Rw, dtype=torch.float64, device=x.device))
            continue
        M = roi_weights(r[1:], H, W, (Rh, Rw), spatial_scale, sampling_ratio, aligned).to(x.device)
        outs.append((x[int(b)].reshape(C, H * W) @ M.t()).reshape(C, Rh, Rw))
    if not outs:
        return torch.zeros(0, C, Rh, Rw, dtype=torch.float64, device=x.device)
    return torch.stack(outs)


class ROIAlign(nn.Module):
    """detectron2.layers.ROIAlign's constructor and call signature over roi_align; returns the input's dtype."""

    def __init__(self, output_size, spatial_scale, sampling_ratio, aligned=True):
        super(ROIAlign, self).__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio
        self.aligned = aligned

    def forward(self, input, rois):
        assert rois.dim() == 2 and rois.size(1) == 5
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio,
                         self.aligned).to(input.dtype)
