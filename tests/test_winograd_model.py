"""CPU model of the Winograd F(2x2, 3x3) arithmetic of kernels_wino.hip in fp32 (input and output transforms in the
kernels' operation order, weights transformed in fp64 and rounded once) reproduces a float64 direct conv to fp32
round-off (the GPU test against the direct kernel is tests/test_gpu_winograd.py)."""
import numpy as np

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]])


def _input_transform(d):            # d [..., 4, 4] -> B^T d B, as wino_input_kernel
    e = np.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :],
                  d[..., 1, :] - d[..., 3, :]], -2)
    return np.stack([e[..., 0] - e[..., 2], e[..., 1] + e[..., 2], e[..., 2] - e[..., 1], e[..., 1] - e[..., 3]], -1)


def _output_transform(m):           # m [..., 4, 4] -> A^T m A, as wino_output_kernel
    u0 = m[..., 0, :] + m[..., 1, :] + m[..., 2, :]
    u1 = m[..., 1, :] - m[..., 2, :] - m[..., 3, :]
    row = lambda u: np.stack([u[..., 0] + u[..., 1] + u[..., 2], u[..., 1] - u[..., 2] - u[..., 3]], -1)
    return np.stack([row(u0), row(u1)], -2)


def _direct(xp, w, dtype):
    H, W = xp.shape[0] - 2, xp.shape[1] - 2
    out = np.zeros((H, W, w.shape[0]), dtype)
    for dy in range(3):
        for dx in range(3):
            out += xp[dy:dy + H, dx:dx + W].astype(dtype) @ w[:, :, dy, dx].T.astype(dtype)
    return out


def test_winograd_f2x2_3x3_fp32_model():
    rs = np.random.RandomState(0)
    H = W = 8
    Cin, Cout = 256, 64
    x = rs.standard_normal((H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    xp = np.pad(x, ((1, 1), (1, 1), (0, 0)))
    V = np.einsum("ai,kcij,bj->abck", G, w.astype(np.float64), G).astype(np.float32)     # [4][4][Cin][Cout]
    win = np.stack([np.stack([xp[2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4] for tx in range(W // 2)]) for ty in range(H // 2)])
    U = _input_transform(np.moveaxis(win, -1, -3))                                       # [ty][tx][Cin][4][4]
    M = np.einsum("yxcab,abck->yxkab", U, V, dtype=np.float32)
    Y = _output_transform(M)                                                             # [ty][tx][Cout][2][2]
    got = np.moveaxis(Y, 2, -1).transpose(0, 2, 1, 3, 4).reshape(H, W, Cout)
    want = _direct(xp, w, np.float64)
    assert np.abs(got - want).max() < 1e-5
