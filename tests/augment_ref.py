"""The augmentation of include/pggan_hip_augment.h restated three times for the tests (test infrastructure):
  * ``apply_loops`` / ``adjoint_loops``: the definition as a literal loop nest over (n, c, i, j), one pixel at a time -- what the numpy
    twin of pggan-pytorch_amd/augment.py is held against with ``==`` (the adjoint as the SCATTER that transposes the forward's gather);
  * ``apply_torch``: the same map as torch index operations in float64, differentiable -- what the step tests insert into the oracle's
    networks (``d_loss_and_grads`` / ``g_loss_and_grads``, after tests/gan_losses_oracle.py);
  * ``pool`` / ``step_table``: the hand-made tables of the kernel tests and the injected tables of the step tests."""
import numpy as np
import torch

import gan_losses_oracle as go

oc = go.oc
FLIP, GAIN = 1, 2


def row(flip=0, dy=0, dx=0, y0=0, y1=0, x0=0, x1=0, gain=None):
    """One table row; ``gain`` None: no gain, a float: the gain flag and its bits."""
    flags = (FLIP if flip else 0) | (GAIN if gain is not None else 0)
    bits = int(np.float32(0.0 if gain is None else gain).view(np.int32))
    return [flags, dy, dx, y0, y1, x0, x1, bits]


def gain_of(r):
    return np.array([r[7]], dtype=np.int32).view(np.float32)[0]


def apply_loops(x, table, channel_mask=0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, C, H, W = x.shape
    out = np.empty_like(x)
    for n in range(N):
        flags, dy, dx, y0, y1, x0, x1 = (int(v) for v in table[n][:7])
        b = gain_of(table[n])
        for c in range(C):
            for i in range(H):
                for j in range(W):
                    if y0 <= i < y1 and x0 <= j < x1:
                        out[n, c, i, j] = np.float32(0.0)
                        continue
                    jp = W - 1 - j if flags & FLIP else j
                    si, sj = i - dy, jp - dx
                    if not (0 <= si < H and 0 <= sj < W):
                        out[n, c, i, j] = np.float32(0.0)
                    elif flags & GAIN and (channel_mask >> c) & 1:
                        out[n, c, i, j] = np.float32(x[n, c, si, sj] + b)
                    else:
                        out[n, c, i, j] = x[n, c, si, sj]
    return out


def adjoint_loops(gy, table):
    """The transpose, as the scatter of the forward's gather: every output pixel that read a source pixel hands its gradient to it (a source
    pixel is read by one output pixel at most, so nothing accumulates)."""
    gy = np.ascontiguousarray(gy, dtype=np.float32)
    N, C, H, W = gy.shape
    gx = np.zeros_like(gy)
    for n in range(N):
        flags, dy, dx, y0, y1, x0, x1 = (int(v) for v in table[n][:7])
        for c in range(C):
            for i in range(H):
                for j in range(W):
                    if y0 <= i < y1 and x0 <= j < x1:
                        continue
                    jp = W - 1 - j if flags & FLIP else j
                    si, sj = i - dy, jp - dx
                    if 0 <= si < H and 0 <= sj < W:
                        gx[n, c, si, sj] = gy[n, c, i, j]
    return gx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pool(H, W, gain=True):
    """The hand-made rows of the kernel tests for images H x W: the identity, every dx mod 4 in both directions, dx = +-(W - 1) and +-W, dy in
    {+-1, +-(H - 1), +-H}, each with the flip on and off, cutouts touching each edge (one pixel, full width, full height, everything, empty),
    and gain rows."""
    rows = [row()]
    dxs = sorted(set([0, 1, 2, 3, -1, -2, -3, 5, -5, W - 1, 1 - W, W, -W, W // 2 + 1]))
    for flip in (0, 1):
        for k, dx in enumerate(dxs):
            rows.append(row(flip=flip, dx=dx, dy=(0, 1, -1)[k % 3]))
        for dy in (1, -1, H - 1, 1 - H, H, -H):
            rows.append(row(flip=flip, dy=dy, dx=flip))
        rows.append(row(flip=flip, y0=0, y1=1, x0=0, x1=1))                          # one pixel in the top left corner
        rows.append(row(flip=flip, dx=1, y0=H - 1, y1=H, x0=W - 1, x1=W))            # ... in the bottom right one
        rows.append(row(flip=flip, dy=1, y0=0, y1=H, x0=W - 2, x1=W))                # full height, at the right edge (a time mask)
        rows.append(row(flip=flip, dx=-2, y0=0, y1=H, x0=0, x1=1))                   # full height, at the left edge
        rows.append(row(flip=flip, dx=3, y0=H - 2, y1=H, x0=0, x1=W))                # full width, at the bottom (a frequency mask)
        rows.append(row(flip=flip, y0=0, y1=1, x0=0, x1=W))                          # full width, at the top
        rows.append(row(flip=flip, dx=1, y0=1, y1=H - 1, x0=1, x1=W - 1))            # the interior
        rows.append(row(flip=flip, y0=0, y1=H, x0=0, x1=W))                          # everything
        rows.append(row(flip=flip, dx=2, y0=2, y1=2, x0=0, x1=W))                    # empty
        if gain:
            rows.append(row(flip=flip, gain=0.25))
            rows.append(row(flip=flip, dx=-1, dy=1, gain=-0.75, y0=0, y1=2, x0=1, x1=3))
            rows.append(row(flip=flip, dx=W - 1, gain=0.0))
    return np.asarray(rows, dtype=np.int32)


def images(N, C, H, W, seed):
    """Random images with -0.0, +0.0, denormals of both signs and large values planted in every plane."""
    rs = np.random.RandomState(seed)
    x = rs.randn(N, C, H, W).astype(np.float32)
    flat = x.reshape(N * C, H * W)
    special = np.array([-0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 3e38, -3e38], dtype=np.float32)
    for p in range(N * C):
        at = rs.permutation(H * W)[:len(special)]
        flat[p, at] = special[:len(at)]
    return x


# ------------------------------------------------------------------------------------------ float64, differentiable
def apply_torch(x, table, channel_mask=0):
    """``x`` [N,C,H,W] (any float dtype, may require grad) under ``table`` as index operations: gather, mask, gain."""
    N, C, H, W = x.shape
    out = []
    i = torch.arange(H).view(H, 1).expand(H, W)
    j = torch.arange(W).view(1, W).expand(H, W)
    chan = torch.tensor([float((channel_mask >> c) & 1) for c in range(C)], dtype=x.dtype).view(C, 1, 1)
    for n in range(N):
        flags, dy, dx, y0, y1, x0, x1 = (int(v) for v in table[n][:7])
        jp = W - 1 - j if flags & FLIP else j
        si, sj = i - dy, jp - dx
        live = (si >= 0) & (si < H) & (sj >= 0) & (sj < W) & ~((i >= y0) & (i < y1) & (j >= x0) & (j < x1))
        y = x[n][:, si.clamp(0, H - 1), sj.clamp(0, W - 1)]
        if flags & GAIN:
            y = y + float(gain_of(table[n])) * chan
        out.append(y * live.to(x.dtype))
    return torch.stack(out)


def step_table(rows, H, W, seed, gain=True):
    """The injected table of a step test: rows that shift, flip, cut and gain, all at once on most images."""
    rs = np.random.RandomState(seed)
    out = []
    for n in range(rows):
        y0, x0 = int(rs.randint(0, H - 2)), int(rs.randint(0, W - 2))
        out.append(row(flip=n % 2, dy=int(rs.randint(-2, 3)), dx=int(rs.randint(-W // 4, W // 4 + 1)), y0=y0, y1=y0 + int(rs.randint(1, 4)),
                       x0=x0, x1=x0 + int(rs.randint(1, W // 2)), gain=float(rs.uniform(-0.3, 0.3)) if gain and n % 3 != 2 else None))
    return np.asarray(out, dtype=np.int32)


def d_loss_and_grads(dparams, gparams, cfg, real, latents, mix, depth, alpha, kind, drift, penalty, weight, table, channel_mask, target=1.0):
    """``gan_losses_oracle.d_loss_and_grads`` with everything D sees augmented: rows [0, N) of ``table`` on the reals, [N, 2N) on G(z); the
    penalty is taken at the augmented images."""
    dp, gp = oc._leafify(go.to64(dparams)), go.to64(gparams)
    real, latents = real.double(), latents.double()
    n = real.size(0)
    real = apply_torch(real, table[:n], channel_mask)
    with torch.no_grad():
        fake = apply_torch(oc.generator_forward(gp, cfg, latents, depth, alpha), table[n:], channel_mask)
    s_r = oc.discriminator_forward(dp, cfg, real, depth, alpha)
    s_f = oc.discriminator_forward(dp, cfg, fake, depth, alpha)
    R = go.real_term(kind, s_r) + drift * s_r ** 2
    F = go.fake_term(kind, s_f)
    total = F + R
    if penalty == 'gp':
        total = total + oc.gradient_penalty(dp, cfg, real, fake, mix.double(), depth, alpha, weight, target).view(n, 1)
    elif penalty == 'r1':
        x = real.detach().requires_grad_(True)
        scores = oc.discriminator_forward(dp, cfg, x, depth, alpha)
        g = torch.autograd.grad(scores.sum(), x, create_graph=True)[0]
        total = total + (0.5 * weight) * g.reshape(n, -1).pow(2).sum(1).view(n, 1)
    else:
        assert penalty is None
    d_cost = total.mean()
    gs = torch.autograd.grad(d_cost, [s_r, s_f], retain_graph=True)
    return dict(d_cost=d_cost.detach(), R=R.detach(), F=F.detach(), s_r=s_r.detach(), s_f=s_f.detach(), grads=go._grads(d_cost, dp),
                bias_terms=float(sum(g.abs().sum() for g in gs)))


def g_loss_and_grads(gparams, dparams, cfg, latents, depth, alpha, kind, table, channel_mask):
    gp, dp = oc._leafify(go.to64(gparams)), go.to64(dparams)
    fake = apply_torch(oc.generator_forward(gp, cfg, latents.double(), depth, alpha), table, channel_mask)
    s = oc.discriminator_forward(dp, cfg, fake, depth, alpha)
    g_cost = go.generator_term(kind, s).mean()
    return dict(g_cost=g_cost.detach(), s=s.detach(), grads=go._grads(g_cost, gp))
