"""numpy restatements of the soft-target loss (sf_ce_mix) and of mixing inside the input step (sf_clip_batch_mix), in
float64 where the kernels compute and in separate float32 operations where they promise float32 bits.

A mix row is 7 int64: partner row, mode (0 none, 1 mixup, 2 CutMix), lam as a float32 bit pattern, y0, x0, y1, x1."""
import numpy as np

MIX_ROW = 7


def lam_bits(lam):
    """The table's column 2 for `lam`: the bit pattern of its float32 value."""
    return int(np.float32(lam).view(np.uint32))


def lam_of(bits):
    return np.uint32(int(bits) & 0xffffffff).view(np.float32)


def make_rows(partner, mode, lam, box=(0, 0, 0, 0)):
    """int64 [N, 7] from per-row partners and per-row or shared mode / lam / box."""
    n = len(partner)
    mode = [mode] * n if np.isscalar(mode) else list(mode)
    lam = [lam] * n if np.isscalar(lam) else list(lam)
    box = [tuple(box)] * n if np.isscalar(box[0]) else [tuple(b) for b in box]
    return np.array([[partner[r], mode[r], lam_bits(lam[r])] + list(box[r]) for r in range(n)], dtype=np.int64)


def row_is_bad(labels, rows, r, K):
    """A label a or b outside [0, K), the partner outside [0, N), lam outside [0, 1] (or high bits set)."""
    n = len(labels)
    a, p, lam = int(labels[r]), r, np.float32(1.0)
    if rows is not None:
        p, bits = int(rows[r, 0]), int(rows[r, 2])
        if not 0 <= p < n or not 0 <= bits <= 0xffffffff:
            return True
        lam = lam_of(bits)
        if not (lam >= 0 and lam <= 1):
            return True
    return not (0 <= a < K and 0 <= int(labels[p]) < K)


def dense_targets(labels, rows, K, eps):
    """t [N, K] float64: (1 - eps) (lam onehot(a) + (1 - lam) onehot(b)) + eps / K; a bad row is all zeros.  `eps` is
    used as given: hand in the float32 value the entry point receives."""
    n = len(labels)
    t = np.zeros((n, K), dtype=np.float64)
    for r in range(n):
        if row_is_bad(labels, rows, r, K):
            continue
        p = r if rows is None else int(rows[r, 0])
        lam = 1.0 if rows is None else float(lam_of(rows[r, 2]))
        t[r, int(labels[r])] += lam
        t[r, int(labels[p])] += 1.0 - lam
        t[r] = (1.0 - eps) * t[r] + eps / K
    return t


def dominant_labels(labels, rows):
    """a when lam >= 0.5, else b (rows that are not bad)."""
    out = np.array(labels, dtype=np.int64).copy()
    if rows is None:
        return out
    for r in range(len(labels)):
        p = int(rows[r, 0])
        if 0 <= p < len(labels) and not float(lam_of(rows[r, 2])) >= 0.5:
            out[r] = labels[p]
    return out


def ce_mix(x, labels, rows, eps):
    """-> (loss, dlogits [N, K], bad rows) in float64: loss = (1 / N) sum_r (logsumexp(x_r) - t_r . x_r),
    dlogits = (softmax - t) / N; a bad row adds nothing and gets a zero gradient row, the divisor stays N."""
    x = np.asarray(x, dtype=np.float64)
    n, K = x.shape
    t = dense_targets(labels, rows, K, eps)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    lse = np.log(s) + m
    bad = np.array([row_is_bad(labels, rows, r, K) for r in range(n)])
    per_row = lse[:, 0] - (t * x).sum(axis=1)
    per_row[bad] = 0.0
    d = (e / s - t) / n
    d[bad] = 0.0
    return per_row.sum() / n, d, int(bad.sum())


def hit_counts(x, labels, rows, k_hi):
    """(top-1 hits, top-k_hi hits) by the integer rule: row r hits iff #{j : x_j > x_l} + #{j < l : x_j == x_l} < k with l
    the dominant label; bad rows and rows holding a NaN or an infinity never hit."""
    x = np.asarray(x)
    n, K = x.shape
    dom = dominant_labels(labels, rows)
    h1 = hk = 0
    for r in range(n):
        if row_is_bad(labels, rows, r, K) or not np.isfinite(x[r]).all():
            continue
        l = int(dom[r])
        rank = int((x[r] > x[r, l]).sum()) + int((x[r, :l] == x[r, l]).sum())
        h1 += rank < 1
        hk += rank < k_hi
    return h1, hk


def mix_batch(x, rows, crop, ph, pw):
    """The mixed batch from the UNMIXED float32 output x [B, T, crop + 2 ph, Wp, C] (what sf_clip_batch writes):
    mode 1 in separate float32 operations — fl(fl(lam * own) + fl(fl(1 - lam) * other)) — and mode 2 by selection
    inside the box, which is in output crop coordinates."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    for b in range(x.shape[0]):
        p, mode = int(rows[b, 0]), int(rows[b, 1])
        lam = lam_of(rows[b, 2])
        y0, x0, y1, x1 = (int(v) for v in rows[b, 3:7])
        if mode == 1:
            rest = np.float32(np.float32(1.0) - lam)
            out[b] = (lam * x[b]).astype(np.float32) + (rest * x[p]).astype(np.float32)
        elif mode == 2:
            out[b, :, ph + y0:ph + y1, pw + x0:pw + x1] = x[p, :, ph + y0:ph + y1, pw + x0:pw + x1]
    return out
