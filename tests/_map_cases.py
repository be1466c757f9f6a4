"""Seeded inputs of the mAP cases: tests/golden/make_golden_map.py records the reference's results for them in
tests/golden/map_vectors.npz (the values only — the inputs are regenerated here from the seed), the tests feed the same
inputs to `get_map` and `sf_map`."""
import numpy as np

SIZES_N = (1, 2, 7, 255, 256, 257, 1000, 2048)
SIZES_C = (1, 17, 33)
SPECIAL = ("neg_column", "zero_tie", "one_class_empty", "all_empty")


def case_names():
    names = ["%s_n%d_c%d" % (kind, n, c) for kind in ("untied", "quant8") for n in SIZES_N for c in SIZES_C]
    return names + list(SPECIAL)


def make_case(name):
    """-> (preds float32 [N, C], labels float32 [N, C])."""
    seed = 1000 + case_names().index(name)
    rs = np.random.RandomState(seed)
    if name in SPECIAL:
        kind, n, c = name, 257, 17
    else:
        kind, n, c = name.split("_")
        n, c = int(n[1:]), int(c[1:])
    if kind == "quant8":
        preds = (np.round(rs.uniform(0.0, 1.0, (n, c)) * 8.0) / 8.0).astype(np.float32)
    else:
        preds = rs.standard_normal((n, c)).astype(np.float32)
    labels = (rs.uniform(0.0, 1.0, (n, c)) < 0.3).astype(np.float32)
    if kind == "neg_column":  # a class nobody predicted: the multi-label TestMeter's reset value, every score tied
        preds[:, 3] = -1e10
        labels[0, 3] = 1.0
    elif kind == "zero_tie":  # -0.0 and +0.0 are ONE threshold
        preds[:, 2] = np.where(rs.uniform(0.0, 1.0, n) < 0.5, np.float32(-0.0), np.float32(0.0))
        preds[::5, 2] = rs.standard_normal(len(preds[::5, 2])).astype(np.float32)
        labels[:4, 2] = (1.0, 0.0, 1.0, 1.0)
    elif kind == "one_class_empty":
        labels[:, 5] = 0.0
    elif kind == "all_empty":
        labels[:] = 0.0
    return preds, labels
