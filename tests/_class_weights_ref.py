"""numpy restatement of sf_class_weights (include/sfhip.h): class weights from per-class support counts.  Checked against
scikit-learn and closed forms in tests/test_weighted_loss_args_cpu.py; the GPU tests compare the kernel with it."""
import numpy as np


def balanced(support):
    """compute_class_weight("balanced") over the classes with support: S / (K+ * support[c]), one float64 division of
    exact integers, rounded once to float32; 0 for a class without support."""
    support = np.asarray(support, dtype=np.int64)
    has = support > 0
    S, kp = int(support[has].sum()), int(has.sum())
    w = np.zeros(support.shape, dtype=np.float64)
    w[has] = np.float64(S) / (np.int64(kp) * support[has]).astype(np.float64)
    return w.astype(np.float32)


def effective(support, beta):
    """(1 - beta) / (1 - beta^support[c]) in float64, rescaled so that the weights over the classes with support sum
    to their number (the sum in class order), rounded once to float32; 0 for a class without support."""
    support = np.asarray(support, dtype=np.int64)
    has = support > 0
    e = np.zeros(support.shape, dtype=np.float64)
    e[has] = (1.0 - beta) / (1.0 - np.power(np.float64(beta), support[has].astype(np.float64)))
    total = 0.0
    for v in e:
        total += float(v)
    scale = float(has.sum()) / total if total > 0.0 else 0.0
    return (e * scale).astype(np.float32)
