"""DeviceModelStats on a whole model (shufflenetv2_cfg1, the smallest model fixture): absent rows before any backward,
the rows of every parameter and gradient around one HipSGD training step against tests/_tensor_stats_ref.py (computed
from .cpu() copies under the op test's rules: integer fields and min / max / absmax exactly, sum and sumsq within
numel * 2^-52 * sum |term|), a second step on the same address table, first_bad after a planted NaN, and record()
captured alone into a graph and replayed."""
import pytest
import torch

import _tensor_stats_ref as ref
from test_gradcam_models_gpu import _build, _case

pytestmark = pytest.mark.gpu
NAME = "shufflenetv2_cfg1"


def _setup():
    z, meta, sd, xs = _case(NAME)
    model = _build(NAME)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model = model.cuda().train()
    labels = torch.from_numpy(z["train/labels"]).long().cuda()
    return model, [x.cuda() for x in xs], labels


def _check(stats, tensors, tag):
    """stats: name -> TensorStats; tensors: name -> GPU tensor, compared through a .cpu() copy."""
    assert list(stats) == list(tensors)
    for name, t in tensors.items():
        ref.check_row(stats[name], ref.ref_row(t.detach().cpu().numpy()), "%s %s" % (tag, name))


def test_a_training_step_under_watch():
    from slowfast.models.step_tail import HipCrossEntropy, HipSGD, StatsRing
    from slowfast.utils.distributed import FlatGradients
    from slowfast.utils.model_stats import DeviceModelStats, first_bad, to_scalars
    model, xs, labels = _setup()
    named = list(model.named_parameters())
    watch = DeviceModelStats(named, slots=4)
    assert watch.names == [n for n, _ in named] and len(named) > 100

    # before any backward: every gradient is absent
    assert all(p.grad is None for _, p in named)
    watch.record("grad")
    got = watch.read("grad")
    assert len(got) == 1 and all(ts.present == 0 and ts.numel == 0 for ts in got[0].values())
    assert watch.rebuilds == {"param": 0, "grad": 1}

    flat = FlatGradients([p for _, p in named])
    opt = HipSGD(model.parameters(), lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)
    loss_fun = HipCrossEntropy(1, StatsRing(4))

    def step():
        flat.zero()
        loss = loss_fun(model(xs), labels)
        loss.backward()
        watch.record("grad")
        opt.step(guard=loss_fun.guard)
        flat.rebind()
        watch.record("param")

    step()
    torch.cuda.synchronize()
    assert watch.rebuilds == {"param": 1, "grad": 2}
    grads, params = watch.read("grad")[-1], watch.read("param")[-1]
    _check(params, {n: p for n, p in named}, "param")
    _check(grads, {n: p.grad for n, p in named}, "grad")  # the optimizer left the gradients in the flat buffer
    assert first_bad(grads) is None and first_bad(params) is None
    sc = to_scalars(grads, "grad")
    assert sc["grad/global/nonfinite"] == 0 and sc["grad/global/norm"] > 0
    want = float(flat.flat.double().norm())
    assert abs(sc["grad/global/norm"] - want) <= 1e-12 * want

    # a second step: the flat gradient buffer keeps the addresses, so neither table is rebuilt
    step()
    torch.cuda.synchronize()
    assert watch.rebuilds == {"param": 1, "grad": 2}
    assert watch.cursor("grad").tolist() == [3, 3] and watch.cursor("param").tolist() == [2, 2]
    again = watch.read("grad")
    assert len(again) == 3 and again[1] == grads and again[2] != grads

    # a NaN planted in one gradient
    victim = named[len(named) // 2][0]
    dict(named)[victim].grad.view(-1)[0] = float("nan")
    watch.record("grad")
    last = watch.read("grad")[-1]
    assert first_bad(last) == victim and last[victim].n_nan == 1
    assert watch.rebuilds["grad"] == 2


def test_record_alone_in_a_captured_graph():
    from slowfast.utils.model_stats import DeviceModelStats
    model, xs, labels = _setup()
    named = list(model.named_parameters())
    watch = DeviceModelStats(named, slots=4)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        watch.record("param")  # eager: builds the address table
    torch.cuda.synchronize()
    eager = watch.ring("param")[0].clone()
    assert watch.cursor("param").tolist() == [1, 1]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        watch.record("param")  # nothing else: the call's two launches, one behind the other
    torch.cuda.synchronize()
    assert watch.cursor("param").tolist() == [1, 1] and watch.rebuilds["param"] == 1  # captured, not run
    with torch.cuda.stream(side):
        graph.replay()
        graph.replay()
    torch.cuda.synchronize()
    assert watch.cursor("param").tolist() == [3, 3]  # advanced by two
    ring = watch.ring("param")
    assert torch.equal(ring[1], eager) and torch.equal(ring[2], eager) and torch.equal(ring[0], eager)
    assert not bool(ring[3].any())  # the slot nobody wrote yet
    got = watch.read("param")
    assert len(got) == 3 and got[0] == got[1] == got[2]
