"""Grad-CAM on the HIP path: the arithmetic of the reference's wdf_visualization/gradcam_video.py (GradVideoCam) for
the two-pathway ResNet models, the single-pathway ResNet and the two efficient backbones the reference tool defaults to
(SlowFastShuffleNet, SlowFastMoibleNetV2).

The reference puts the model in eval(), walks model._modules child by child, hooks the gradient of the [slow, fast]
pair behind a chosen child, back-propagates a one-hot class vector from the head's eval output (:107-157) and builds
one class-activation map per frame and pathway (:159-211).  Here the eval forward runs once under
engine.eval_taping(target): everything up to the target child is the plain eval forward, everything after it records
activation-gradient closures (folded conv epilogues through sf_epilogue_bwd / sf_epilogue_bwd_act, depthwise convs with
their epilogue through sf_dwconv_dgrad_epi, the head's softmax-mean through sf_head_act_mean_bwd), and the replay hands back d out[n, cls[n]] / d (target outputs).  No weight-gradient kernel
runs and no parameter's .grad is touched."""
import torch

import sfhip
from . import engine

_TWO_PATHWAY = ("s1", "s1_fuse", "s2", "s2_fuse", "s3", "s3_fuse", "s4", "s4_fuse", "s5")
_ONE_PATHWAY = ("s1", "s2", "s3", "s4", "s5")


def target_layers(model):
    """Names of the top-level children whose outputs class_gradients can differentiate to (the children in front of
    `head`; the identity pathway{p}_pool children are not targets).  Raises NotImplementedError for a model the
    eval-mode tape does not cover."""
    from .custom_video_model_builder import SlowFastDualAttention, SlowFastMoibleNetV2, SlowFastShuffleNet
    from .video_model_builder import ResNet, SlowFast
    if not isinstance(model, (SlowFast, SlowFastDualAttention, ResNet, SlowFastShuffleNet, SlowFastMoibleNetV2)):
        raise NotImplementedError(
            "Grad-CAM on the HIP path covers SlowFast, SlowFastDualAttention, ResNet, SlowFastShuffleNet and "
            "SlowFastMoibleNetV2; %s has no eval-mode backward" % type(model).__name__)
    if getattr(model, "enable_detection", False):
        raise NotImplementedError("Grad-CAM on the HIP path does not cover DETECTION.ENABLE models (ResNetRoIHead)")
    if isinstance(model, (SlowFastShuffleNet, SlowFastMoibleNetV2)):  # forward = the registered children in order
        names = [n for n, _ in model.named_children()]
        return tuple(names[:names.index("head")])
    return _ONE_PATHWAY if isinstance(model, ResNet) else _TWO_PATHWAY


def _class_gradients(model, inputs, target_layer, target_class):
    """class_gradients with acts / grads as NDHWC Acts (the layout the CAM kernels read)."""
    valid = target_layers(model)
    if target_layer not in valid:
        raise ValueError("unknown target layer %r for %s: valid targets are %s" % (
            target_layer, type(model).__name__, ", ".join(valid)))
    inputs = list(inputs)
    if any(not isinstance(x, torch.Tensor) for x in inputs):
        raise TypeError("class_gradients takes NCTHW tensors (PackedClip inputs are not supported)")
    was_training = model.training
    if was_training:
        model.eval()
    try:
        with torch.no_grad(), engine.eval_taping(target_layer) as t:
            out = engine.run_model(model, inputs)
            n, k = out.shape
            if target_class is None:
                cls = out.argmax(dim=1)
            else:
                cls = torch.as_tensor(target_class, dtype=torch.int64, device=out.device).reshape(-1).expand(n)
            dout = torch.zeros((n, k), dtype=torch.float32, device=out.device)
            dout.scatter_(1, cls.reshape(n, 1), 1.0)
            acts = list(t.target_acts)
            grads = t.backward(dout)
    finally:
        if was_training:
            model.train()
    return acts, grads, out, cls.contiguous()


def class_gradients(model, inputs, target_layer, target_class=None):
    """(acts, grads, out, cls) of one eval forward of `model` on `inputs` (the list of NCTHW clips it takes, any batch):
      acts   the outputs of the top-level child `target_layer`, one NCTHW fp32 tensor per pathway;
      grads  d out[n, cls[n]] / d acts, same shapes;
      out    the eval output [N, classes] (head activation applied, mean over T,H,W: what model.eval()(inputs) returns);
      cls    target_class (int or [N] tensor / sequence) as an int64 [N] tensor on the device, or the per-sample argmax
             of `out` when None (gradcam_video.py:143-147).
    The model is evaluated in eval mode whatever its current mode (restored afterwards).  Nothing is synchronised with
    the host: the one-hot upstream gradient is scattered on the device.  No parameter gradient is computed and every
    p.grad is left as it was."""
    acts, grads, out, cls = _class_gradients(model, inputs, target_layer, target_class)
    with torch.no_grad():
        return [sfhip.to_ncthw(a) for a in acts], [sfhip.to_ncthw(g) for g in grads], out, cls


class GradVideoCam(object):
    """Counterpart of the reference's GradVideoCam (gradcam_video.py:84-211) up to its host-side post-processing.

    generate_cam_videos returns, per pathway, the fp32 maps the reference computes at :159-179 / :193-211 BEFORE it
    quantises them to uint8 and resizes them with PIL (both stay the caller's host work).  Per sample n, pathway p and
    frame t, with A the target activations and G their gradients:
        w[c] = mean_{h,w} G[n,c,t,h,w];  Abar[c,h,w] = mean_t A[n,c,t,h,w];
        cam = max(0, 1 + sum_c w[c] * Abar[c]);  cam = (cam - min) / (max - min) over the frame.
    Deviation: a frame whose range max - min is zero gives zeros here; the reference divides by zero there (NaN)."""

    def __init__(self, model, target_layer):
        self.model = model
        self.target_layer = target_layer
        valid = target_layers(model)
        if target_layer not in valid:
            raise ValueError("unknown target layer %r for %s: valid targets are %s" % (
                target_layer, type(model).__name__, ", ".join(valid)))
        self.model.eval()  # as the reference's constructor does (:89)

    def generate_cam_videos(self, inputs, target_class=None):
        """[slow_cams, fast_cams] (one entry for ResNet): fp32 device tensors [N, T_p, H_p, W_p] in [0, 1]."""
        acts, grads, _, _ = _class_gradients(self.model, inputs, self.target_layer, target_class)
        return [sfhip.cam_map(a, sfhip.cam_weights(g)) for a, g in zip(acts, grads)]
