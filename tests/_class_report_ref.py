"""Brute-force restatement of sf_confusion_update / sf_class_report (include/sfhip.h): a loop over the rows, `sorted`
with the documented tie rule, Python integer counts and one `float` division per ratio.  Nothing is vectorised, so that
it is obviously right; the kernels and the meter are compared with it.

The rule of a row: class j stands in front of class c iff x[j] > x[c], or x[j] == x[c] and j < c (values compare as
floats: -0.0 ties +0.0).  The order of a row is therefore `sorted` by (-value, index); its first class is the predicted
one and the label is within the top k iff its position is below k.  A row with a label outside [0, K) is refused
(refused[0]); a row with a valid label that holds a NaN or an infinity is refused (refused[1]); a refused row adds to
nothing else."""
import math

PER_CLASS_COLUMNS = ("support", "precision", "recall", "f1", "top1_acc", "topk_acc")
SUMMARY_FIELDS = ("samples", "accuracy", "mean_class_accuracy", "macro_precision", "macro_recall", "macro_f1",
                  "classes_with_support", "classes_never_predicted")


def empty_counts(K):
    return {"conf": [[0] * K for _ in range(K)], "hits": [[0, 0] for _ in range(K)], "refused": [0, 0]}


def row_order(row):
    """Class indices of one row, best first: by value descending, equal values by index ascending."""
    vals = [float(v) for v in row]
    # -0.0 and +0.0 are equal as floats; `0.0 - v` maps both to a zero, and zeros compare equal whatever their sign
    return sorted(range(len(vals)), key=lambda j: (0.0 - vals[j], j))


def confusion_update(counts, preds, labels, k_hi):
    """Add the rows of `preds` ([N][K] numbers) with `labels` ([N] integers) to `counts`; returns `counts`."""
    K = len(counts["conf"])
    assert 1 <= k_hi <= K
    for row, label in zip(preds, labels):
        label = int(label)
        assert len(row) == K
        if label < 0 or label >= K:
            counts["refused"][0] += 1
            continue
        if any(math.isnan(float(v)) or math.isinf(float(v)) for v in row):
            counts["refused"][1] += 1
            continue
        order = row_order(row)
        counts["conf"][label][order[0]] += 1
        position = order.index(label)
        if position < 1:
            counts["hits"][label][0] += 1
        if position < k_hi:
            counts["hits"][label][1] += 1
    return counts


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else 0.0


def class_report(counts):
    """(summary: dict of SUMMARY_FIELDS, per_class: [K][6] in PER_CLASS_COLUMNS order) of `counts`."""
    conf, hits = counts["conf"], counts["hits"]
    K = len(conf)
    table = []
    samples = correct = with_support = never = 0
    sum_p = sum_r = sum_f = 0.0
    for c in range(K):
        support = sum(conf[c][j] for j in range(K))
        predicted = sum(conf[j][c] for j in range(K))
        tp = conf[c][c]
        fp, fn = predicted - tp, support - tp
        p, r, f = _ratio(tp, tp + fp), _ratio(tp, tp + fn), _ratio(2 * tp, 2 * tp + fp + fn)
        table.append([float(support), p, r, f, _ratio(hits[c][0], support), _ratio(hits[c][1], support)])
        samples += support
        correct += tp
        if predicted == 0:
            never += 1
        if support > 0:
            with_support += 1
            sum_p += p
            sum_r += r
            sum_f += f
    summary = {"samples": samples, "accuracy": _ratio(correct, samples),
               "mean_class_accuracy": _ratio(sum_r, with_support), "macro_precision": _ratio(sum_p, with_support),
               "macro_recall": _ratio(sum_r, with_support), "macro_f1": _ratio(sum_f, with_support),
               "classes_with_support": with_support, "classes_never_predicted": never}
    return summary, table


def topk_hits(preds, labels, k):
    """Rows whose label is within the top k by the same rule, refused rows counting as misses (what sf_topk_errors
    counts)."""
    n = 0
    for row, label in zip(preds, labels):
        label = int(label)
        if label < 0 or label >= len(row) or any(math.isnan(float(v)) or math.isinf(float(v)) for v in row):
            continue
        n += 1 if row_order(row).index(label) < k else 0
    return n
