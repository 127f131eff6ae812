"""torch-CPU statement of the sliced Wasserstein metric (Karras et al. 2018, section 5), the reference the device path
(pggan-pytorch_amd/csrc/swd.hip, metrics.SlicedWasserstein) is held against.  Every function takes its dtype from its input, so
the same code is the fp32 reference of a single kernel and the fp64 adjudicator of the whole metric.

  1. Laplacian pyramid: 5x5 binomial filter, reflect boundary without the edge sample (F.pad 'reflect'), grouped conv2d;
  2. descriptors: 3x7x7 slices around given (x, y) centres, rows in (channel, dy, dx) order;
  3. per-channel normalisation over (descriptor, dy, dx), population standard deviation;
  4. projections on unit directions, torch.sort, mean absolute difference; reported x 1000."""
import torch
import torch.nn.functional as F

_F1 = [1.0, 4.0, 6.0, 4.0, 1.0]


def _conv5(x, gain):
    f = torch.tensor(_F1, dtype=torch.float64) / 16.0
    k = (torch.outer(f, f) * gain).to(x.dtype)
    c = x.shape[1]
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode='reflect'), k[None, None].repeat(c, 1, 1, 1), groups=c)


def down(x):
    return _conv5(x, 1.0)[:, :, ::2, ::2]


def up(x):
    n, c, h, w = x.shape
    z = torch.zeros(n, c, 2 * h, 2 * w, dtype=x.dtype)
    z[:, :, ::2, ::2] = x
    return _conv5(z, 4.0)


def lap_pyramid(x, min_size=16):
    g = [x]
    while g[-1].shape[-1] > min_size:
        g.append(down(g[-1]))
    return [g[i] - up(g[i + 1]) for i in range(len(g) - 1)] + [g[-1]]


def descriptors(level, centres, P):
    """level [N,3,S,S], centres int [N*P,2] of (x, y) -> [N*P,3,7,7]"""
    out = torch.empty(centres.shape[0], level.shape[1], 7, 7, dtype=level.dtype)
    for j in range(centres.shape[0]):
        x, y = int(centres[j, 0]), int(centres[j, 1])
        out[j] = level[j // P, :, y - 3:y + 4, x - 3:x + 4]
    return out


def normalize(desc):
    """[M,3,7,7] -> normalised rows [M,147]"""
    d = desc - desc.mean(dim=(0, 2, 3), keepdim=True)
    d = d / d.std(dim=(0, 2, 3), keepdim=True, unbiased=False)
    return d.reshape(d.shape[0], -1)


def sliced_distance(a, b, directions):
    """a, b [M,147] normalised; directions [R,147,K] -> mean over R of mean |sort(a @ D) - sort(b @ D)|"""
    vals = []
    for d in directions.to(a.dtype):
        pa = (a @ d).sort(dim=0)[0]
        pb = (b @ d).sort(dim=0)[0]
        vals.append((pa - pb).abs().mean())
    return float(sum(vals) / len(vals))


def swd(real, fake, centres, directions, P):
    """The whole metric: real, fake [N,3,R,R]; centres: one int [N*P,2] tensor per level (used for both sets).
    Returns {'swd': [value x 1000 per level], 'mean': ...}."""
    lr, lf = lap_pyramid(real), lap_pyramid(fake)
    vals = []
    for li in range(len(lr)):
        a = normalize(descriptors(lr[li], centres[li], P))
        b = normalize(descriptors(lf[li], centres[li], P))
        vals.append(sliced_distance(a, b, directions) * 1e3)
    return {'swd': vals, 'mean': sum(vals) / len(vals)}
