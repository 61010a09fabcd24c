"""fp64 reference side of the position-embedding resampling tests: the target (torch's F.interpolate, bicubic,
antialias=True, align_corners=False, in fp64), its per-axis weight matrix extracted from an identity, and the element
bound the fp32 kernels are held to.  Pure CPU; shared by test_pos_resample_ref.py, test_gpu_pos_resample.py and
test_gpu_dynamic_size.py."""
import numpy as np
import torch
import torch.nn.functional as F

# (g, g2): enlarging, shrinking (6 and 8 taps), clipped rows, non-integer ratios, grid 1, and Base at 224 -> 288
GRIDS = [(4, 7), (7, 4), (4, 6), (5, 2), (7, 10), (14, 7), (2, 5), (1, 3), (28, 36)]
U = 2.0 ** -24   # unit roundoff of fp32


def interpolate(img, size, antialias=True, align_corners=False):
    return F.interpolate(img, size=size, mode="bicubic", align_corners=align_corners, antialias=antialias)


def torch_matrix(g, g2, antialias=True, align_corners=False):
    """W fp64 [g2, g] of one axis: torch's resize of the g unit vectors (a [1, g, 1, g] image, width g -> g2)."""
    eye = torch.eye(g, dtype=torch.float64).reshape(1, g, 1, g)
    return interpolate(eye, (1, g2), antialias, align_corners)[0, :, 0, :].T.contiguous().numpy()


def target(p, g, g2, antialias=True, align_corners=False):
    """p fp64 tensor [g*g, C] -> [g2*g2, C]: the operator the kernels implement, by torch in fp64 (differentiable)."""
    C = p.shape[1]
    img = p.reshape(1, g, g, C).permute(0, 3, 1, 2)
    return interpolate(img, (g2, g2), antialias, align_corners).permute(0, 2, 3, 1).reshape(g2 * g2, C)


def apply_matrices(Wy, Wx, p, n_src):
    """(Wy (x) Wx) p in fp64 numpy: p [n_src*n_src, C] -> [rows(Wy)*rows(Wx), C]."""
    C = p.shape[1]
    rows = np.tensordot(Wy, p.reshape(n_src, n_src, C), axes=(1, 0))        # [a, x, c]
    out = np.tensordot(Wx, rows, axes=(1, 1)).transpose(1, 0, 2)             # [b, a, c] -> [a, b, c]
    return np.ascontiguousarray(out).reshape(-1, C)


def element_bound(rows, n_src, p):
    """(taps_y * taps_x + 3) * 2^-24 * sum |w_y| |w_x| |p| per output element, fp64 numpy [n_dst*n_dst, C].  `rows` is the
    host table (nvit_amd.resample Rows) of the direction under test, p its fp64 input [n_src*n_src, C].  One rounding per
    product and per add of the taps_y * taps_x terms, one for the product of the two weights, one each for rounding the two
    fp64 weights to fp32: first-order, derived, not measured."""
    from nvit_amd import resample as R
    A = np.abs(R.dense(rows, n_src))
    taps = np.array([len(w) for w in rows[1]], dtype=np.float64)
    S = apply_matrices(A, A, np.abs(p), n_src)
    n = (taps[:, None] * taps[None, :] + 3.0).reshape(-1, 1)
    return n * U * S


def fp32_evaluation(rows, n_src, p):
    """What a plain fp32 evaluation in the kernels' order gives (numpy float32, no FMA): the CPU stand-in for the kernel in
    the rejection check."""
    first, weights = rows
    n_dst = len(first)
    C = p.shape[1]
    src = p.astype(np.float32).reshape(n_src, n_src, C)
    out = np.zeros((n_dst, n_dst, C), dtype=np.float32)
    w32 = [np.asarray(w, dtype=np.float64).astype(np.float32) for w in weights]
    for dy in range(n_dst):
        for dx in range(n_dst):
            acc = np.zeros(C, dtype=np.float32)
            for iy, wy in enumerate(w32[dy]):
                for ix, wx in enumerate(w32[dx]):
                    w = np.float32(wy * wx)
                    acc = (acc + w * src[first[dy] + iy, first[dx] + ix]).astype(np.float32)
            out[dy, dx] = acc
    return out.reshape(-1, C)
