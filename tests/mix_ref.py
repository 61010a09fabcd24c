"""numpy restatement of the on-device Mixup / CutMix: the draw, the apply and the soft target.

Independent of nvit_amd/mix.py and of the kernels on purpose: the GPU tests compare both against this file.  The only
thing it takes from outside is the Beta quantile table, as an argument: tests/test_mix_ref.py pins the product's table
to scipy.

Semantics.  Rows p and B-1-p of the batch are pair p (timm's `pair` mode); the middle row of an odd batch is its own
partner and is never mixed.  One Philox4x32-10 call per pair, key = (seed low, seed high ^ DOMAIN), counter =
(first_index + p, step); the four words are the gate, the Mixup/CutMix switch, lambda's quantile and the box centre."""
import numpy as np

from augment_ref import philox4x32_10

DOMAIN = 0x4D495821
KNOTS = 1024
NONE, MIXUP, CUTMIX = 0, 1, 2
M32 = np.uint64(0xFFFFFFFF)


def philox_vec(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint64 arrays holding 32-bit values); one key."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(seed, step, first_index, npairs):
    """The four 32-bit words of pairs 0..npairs-1, as uint64 arrays."""
    g = np.array([first_index + p for p in range(npairs)], dtype=np.uint64)
    n = np.ones(npairs, dtype=np.uint64)
    return philox_vec(g & M32, g >> np.uint64(32), n * np.uint64(step & 0xFFFFFFFF), n * np.uint64(step >> 32),
                      seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ DOMAIN)


def lam_of(r2, q):
    """lambda from the quantile table q (1025 values; used in fp32): linear between knots, multiply then add."""
    q = np.asarray(q, dtype=np.float32)
    u = (r2 >> np.uint64(8)).astype(np.int64)
    k = u >> 14
    f = (u & 0x3FFF).astype(np.float32) * np.float32(2.0 ** -14)
    return (q[k] + (f * (q[k + 1] - q[k])).astype(np.float32)).astype(np.float32)


def draw_pairs(seed, step, first_index, npairs, H, W, q_mix, q_cut, prob=1.0, switch_prob=0.5):
    """Per pair: mode [n] int, lam [n] float32, box [n,4] int (y0, y1, x0, x1).  q_mix / q_cut: the quantile table of
    the mode's alpha, None = mode off."""
    r0, r1, r2, r3 = words(seed, step, first_index, npairs)
    unit = np.float32(2.0 ** -24)
    gate = (r0 >> np.uint64(8)).astype(np.float32) * unit < np.float32(prob)
    sw = (r1 >> np.uint64(8)).astype(np.float32) * unit < np.float32(switch_prob)
    mode = np.zeros(npairs, dtype=np.int64)
    lam = np.ones(npairs, dtype=np.float32)
    box = np.zeros((npairs, 4), dtype=np.int64)
    if q_mix is None and q_cut is None:
        return mode, lam, box
    cut = np.ones(npairs, bool) if q_mix is None else (np.zeros(npairs, bool) if q_cut is None else sw)
    if q_mix is not None:
        m = gate & ~cut
        mode[m], lam[m] = MIXUP, lam_of(r2, q_mix)[m]
    if q_cut is not None:
        m = gate & cut
        l = lam_of(r2, q_cut)
        cy = (((r3 & np.uint64(0xFFFF)) * np.uint64(H)) >> np.uint64(16)).astype(np.int64)
        cx = (((r3 >> np.uint64(16)) * np.uint64(W)) >> np.uint64(16)).astype(np.int64)
        ratio = np.sqrt((np.float32(1.0) - l).astype(np.float64))
        cut_h, cut_w = (H * ratio).astype(np.int64), (W * ratio).astype(np.int64)
        y0, y1 = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
        x0, x1 = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        lc = (1.0 - ((y1 - y0) * (x1 - x0)).astype(np.float64) / np.float64(H * W)).astype(np.float32)
        mode[m], lam[m] = CUTMIX, lc[m]
        box[m] = np.stack([y0, y1, x0, x1], axis=1)[m]
    return mode, lam, box


def draw(seed, step, first_index, y, H, W, q_mix, q_cut, prob=1.0, switch_prob=0.5):
    """What nvit_mix_draw writes: (table int32 [B,8], lam float32 [B], y2 int64 [B])."""
    y = np.asarray(y, dtype=np.int64)
    B = len(y)
    mode, lam, box = draw_pairs(seed, step, first_index, (B + 1) // 2, H, W, q_mix, q_cut, prob, switch_prob)
    table = np.zeros((B, 8), dtype=np.int32)
    lam_rows = np.ones(B, dtype=np.float32)
    for p in range((B + 1) // 2):
        i, j = p, B - 1 - p
        if i == j:   # the middle row
            table[i] = [NONE, np.float32(1.0).view(np.int32), 0, 0, 0, 0, i, 0]
            continue
        for b, partner in ((i, j), (j, i)):
            table[b] = [mode[p], lam[p:p + 1].view(np.int32)[0], *box[p], partner, 0]
            lam_rows[b] = lam[p]
    return table, lam_rows, y[table[:, 6]]


def apply(X, table):
    """What nvit_mix_apply writes: X float32 [B,C,H,W], table int [B,8]."""
    X = np.asarray(X, dtype=np.float32)
    out = X.copy()
    for b in range(X.shape[0]):
        mode, lam_bits, y0, y1, x0, x1, j = (int(v) for v in table[b, :7])
        if j == b or mode == NONE:
            continue
        lam = np.array([lam_bits], dtype=np.int32).view(np.float32)[0]
        if mode == MIXUP:
            om = np.float32(1.0) - lam
            out[b] = (lam * X[b]).astype(np.float32) + (om * X[j]).astype(np.float32)
        else:
            out[b, :, y0:y1, x0:x1] = X[j, :, y0:y1, x0:x1]
    return out


def soft_target(y, y2, lam, smoothing, N):
    """timm's mixup_target in fp64: [B,N]."""
    y, y2, lam = np.asarray(y), np.asarray(y2), np.asarray(lam, dtype=np.float64)
    B = len(y)
    t = np.zeros((B, N))
    np.add.at(t, (np.arange(B), y), lam)
    np.add.at(t, (np.arange(B), y2), 1.0 - lam)
    return (1.0 - smoothing) * t + smoothing / N


__all__ = ["philox4x32_10", "philox_vec", "words", "lam_of", "draw_pairs", "draw", "apply", "soft_target"]
