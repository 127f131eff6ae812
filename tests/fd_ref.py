"""TEST INFRASTRUCTURE: the Frechet distance over the random embedding, restated for the CPU (include/pggan_hip_embed.h, DESIGN.md
section 7).  numpy float32 twins of the three ends of the embedding (one rounding per operation, the kernels' order: compared with ==),
the 3x3 layer in fp64 from bf16 operands (tests/sampling_ref.py), the moments with exactly rounded sums (math.fsum) and the statistic by
another route than the product's (the eigenvalues of cov1 cov2).  bf16 tensors are uint16 bit patterns here, as in the C-ABI."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import sampling_ref

STEM_CH = 8
SLOPE, EPS = 0.2, 1e-8


# --------------------------------------------------------------------------------------------------------------------- bf16 <-> fp32
def rne_bits(x):
    """float32 array of finite values -> uint16 bf16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f32_of(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bits_of_tensor(t):
    """A bf16 torch tensor (any device) -> its uint16 bit patterns as numpy."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def tensor_of_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------------- the ends
def stem(x_u8):
    """uint8 [M,C,H,W] -> bits [M,H,W,8]: rne((float(x) - 127.5f) / 127.5f), zeros above C."""
    x = np.asarray(x_u8)
    M, C, H, W = x.shape
    v = (x.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    out = np.zeros((M, H, W, STEM_CH), dtype=np.uint16)
    out[..., :C] = rne_bits(v).transpose(0, 2, 3, 1)
    return out


def pool2(bits):
    """bits [N,H,W,Ch] -> bits [N,H/2,W/2,Ch]: rne(((a00 + a01) + (a10 + a11)) * 0.25f) in float32."""
    a = f32_of(bits)
    s = (a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + (a[:, 1::2, 0::2] + a[:, 1::2, 1::2])
    return rne_bits(s * np.float32(0.25))


def gap(bits):
    """bits [N,H,W,Ch] -> float32 [N,Ch]: the sum over (h, w) in row-major order from 0.0f, times 1.0f / (H W)."""
    a = f32_of(bits)
    N, H, W, Ch = a.shape
    s = np.zeros((N, Ch), dtype=np.float32)
    for h in range(H):
        for w in range(W):
            s = s + a[:, h, w]
    return s * (np.float32(1.0) / np.float32(H * W))


# ---------------------------------------------------------------------------------------------------------------------- the network
def width(H):
    return min(128, 4096 // H)


def layers(r):
    out, cin = [], STEM_CH
    while r >= 4:
        out.append((r, cin, width(r)))
        cin, r = width(r), r // 2
    return out


def weights(seed, H, cin):
    """The layer's weights in the stored layout [3,3,Cout,Cin], fp64 values on the bf16 grid."""
    g = torch.Generator().manual_seed(seed * 1000003 + H)
    w = torch.randn(width(H), cin, 3, 3, generator=g).permute(2, 3, 0, 1).contiguous()
    return w.to(torch.bfloat16).double()


def layer(a_bits, wb, dtype, rounded=True):
    """One 3x3 layer of the embedding from its bf16 input (bits [N,H,W,Cin]) in ``dtype``: [N,H,W,Cout] of that dtype.  The sum runs
    over 32-channel blocks, as in tests/test_sampling_gpu.py: nothing worth naming in fp64, and in float32 still a torch CPU evaluation
    of the layer, with the error of a blocked sum (torch's one-call float32 conv at K = 1152 misses the criterion's own condition)."""
    x = torch.from_numpy(f32_of(a_bits).copy()).to(dtype).permute(0, 3, 1, 2)
    w = wb.to(dtype).permute(2, 3, 0, 1)
    cin = x.shape[1]
    v = sum(F.conv2d(x[:, i:i + 32], w[:, i:i + 32], None, 1, 1) for i in range(0, cin, 32))
    v = torch.tensor(math.sqrt(2.0 / (9 * cin)), dtype=dtype) * v
    v = torch.where(v > 0, v, v * SLOPE)
    v = sampling_ref.pixelnorm(v, EPS).permute(0, 2, 3, 1).contiguous()
    return sampling_ref.rne_bf16(v) if rounded else v


def embed(x_u8, seed=0):
    """uint8 [n,C,r,r] -> float32 features [n,128]: the whole chain, every layer in fp64 and rounded once."""
    bits = stem(x_u8)
    for H, cin, _ in layers(x_u8.shape[-1]):
        y = layer(bits, weights(seed, H, cin), torch.float64)
        bits = rne_bits(y.float().numpy())                             # (already on the bf16 grid: exact)
        if H > 4:
            bits = pool2(bits)
    return gap(bits)


# ---------------------------------------------------------------------------------------------------------------------- the moments
def mean_exact(x):
    """Column means of a float32 matrix: exactly rounded sums, one division."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.fsum(x[:, f]) for f in range(x.shape[1])]) / x.shape[0]


def cov_exact(x, mean):
    """(cov, mag): sum_r a_ri a_rj / (M - 1) with a = (double)x - mean, every sum exactly rounded (the products are rounded once), and
    mag = sum_r |a_ri a_rj| for the summation bound."""
    a = np.asarray(x, dtype=np.float64) - np.asarray(mean, dtype=np.float64)
    M, F = a.shape
    cov, mag = np.empty((F, F)), np.empty((F, F))
    for i in range(F):
        p = a[:, i:i + 1] * a[:, i:]
        for j in range(i, F):
            cov[i, j] = cov[j, i] = math.fsum(p[:, j - i]) / (M - 1)
        m = np.abs(p).sum(axis=0)
        mag[i, i:] = m
        mag[i:, i] = m
    return cov, mag


def moments(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    a = x - mean
    return mean, a.T.dot(a) / (x.shape[0] - 1)


def frechet(mu1, cov1, mu2, cov2):
    """|mu1 - mu2|^2 + tr cov1 + tr cov2 - 2 tr (cov1 cov2)^(1/2) from the eigenvalues of the (unsymmetric) product cov1 cov2."""
    lam = np.linalg.eigvals(np.asarray(cov1).dot(cov2)).real
    return float(((np.asarray(mu1) - mu2) ** 2).sum() + np.trace(cov1) + np.trace(cov2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


# --------------------------------------------------------------------------------------------------------------------- synthetic sets
def box_images(n, C, r, passes, seed):
    """uint8 [n,C,r,r]: seeded white noise, box-filtered (3x3, wrap-around) ``passes`` times with the contrast restored after every pass."""
    x = np.random.RandomState(seed).rand(n, C, r, r) - 0.5
    for _ in range(passes):
        x = 3.0 * sum(np.roll(np.roll(x, dy, axis=2), dx, axis=3) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return np.clip(np.round((x + 0.5) * 255.0), 0, 255).astype(np.uint8)
