"""NDB/k and JSD over k-means bins (Richardson & Weiss 2018), restated for the CPU independently of the product's
numpy twin (pggan-pytorch_amd/metrics.py): one image at a time, distances and sums as Python integers, the statistic with math.* on
Python floats.  Slow and plain on purpose; the tests use it at sizes where that does not matter.

  split      held = the first h of torch.randperm(M) seeded seed, fit = the rest
  init       centroids = copies of the first K images of fit[torch.randperm(len(fit)) seeded seed + 1]
  assign     label[m] = the lowest k with the smallest sum_d (X[m,d] - c[k,d])^2
  update     c[k,d] = (2 sum + n) // (2 n) over the fit-set members of bin k; n = 0 keeps the centroid
  stop       an assignment whose fit-set labels equal the previous one's (converged), or max_iter assignments, each but a converging one
             followed by an update; an unconverged fit assigns once more to the final centroids
  counts     ref = labels of the held-out images (of the fit set when h = 0); gen = labels of the generated images
  statistic  z-test of two proportions per bin with the pooled standard error (se = 0: z = 0), JSD in bits"""
import math

import numpy as np
import torch

Z_05 = 1.959963984540054


def planted_centres(blobs, C, r, seed):
    """``blobs`` random images [blobs,C,r,r] with levels in 40 .. 215: the modes of a planted distribution."""
    return np.random.RandomState(seed).randint(40, 216, size=(blobs, C, r, r))


def planted_images(centres, per_blob, seed, spread=12, drop=()):
    """``per_blob`` uint8 images around every centre (uniform noise of +-``spread`` levels per byte), the blobs in ``drop`` left out, in
    a seeded random order: two calls with the same centres and different seeds are two samples of one distribution."""
    rs = np.random.RandomState(seed)
    out = []
    for b in range(centres.shape[0]):
        noise = rs.randint(-spread, spread + 1, size=(per_blob,) + centres.shape[1:])
        if b not in drop:
            out.append(np.clip(centres[b][None] + noise, 0, 255).astype(np.uint8))
    x = np.concatenate(out)
    return x[rs.permutation(x.shape[0])]


def split(M, h, seed):
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(seed)).tolist()
    return perm[:h], perm[h:]


def initial(fit, K, seed):
    perm = torch.randperm(len(fit), generator=torch.Generator().manual_seed(seed + 1)).tolist()
    return [fit[i] for i in perm[:K]]


def sqdist(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def assign(x, c):
    """(labels, distances): lists of Python ints, one image at a time."""
    M, K = x.shape[0], c.shape[0]
    xf, cf = x.reshape(M, -1), c.reshape(K, -1)
    labels, dists = [], []
    for m in range(M):
        best_k, best = 0, sqdist(xf[m], cf[0])
        for k in range(1, K):
            d = sqdist(xf[m], cf[k])
            if d < best:
                best_k, best = k, d
        labels.append(best_k)
        dists.append(best)
    return labels, dists


def sums(x, labels, K):
    """(sums [K, ...] int64, counts list); a label of -1 is no member."""
    s = np.zeros((K,) + x.shape[1:], dtype=np.int64)
    n = [0] * K
    for m, k in enumerate(labels):
        if k >= 0:
            s[k] += x[m]
            n[k] += 1
    return s, n


def centroids(s, n, previous):
    out = previous.copy()
    for k in range(len(n)):
        if n[k] > 0:
            flat = [(2 * int(v) + n[k]) // (2 * n[k]) for v in s[k].reshape(-1)]
            out[k] = np.array(flat, dtype=np.int64).reshape(s[k].shape).astype(np.uint8)
    return out


def fit(x, K, h=0, seed=0, max_iter=30):
    held, fitset = split(x.shape[0], h, seed)
    in_fit = set(fitset)
    c = x[initial(fitset, K, seed)].copy()
    prev, iterations, converged = None, 0, False
    while iterations < max_iter:
        labels, _ = assign(x, c)
        iterations += 1
        members = [k if m in in_fit else -1 for m, k in enumerate(labels)]
        if members == prev:
            converged = True
            break
        s, n = sums(x, members, K)
        c = centroids(s, n, c)
        prev = members
    if not converged:
        labels, _ = assign(x, c)
    ref = [0] * K
    for m in (held if h else fitset):
        ref[labels[m]] += 1
    return {'centroids': c, 'labels': labels, 'ref': ref, 'iterations': iterations, 'converged': converged, 'held': held, 'fit': fitset}


def histogram(images, c):
    gen = [0] * c.shape[0]
    for k in assign(images, c)[0]:
        gen[k] += 1
    return gen


def statistic(ref, gen, z_threshold=Z_05):
    K, P, Q = len(ref), sum(ref), sum(gen)
    z, ndb, jsd = [], 0, 0.0
    kl_p = kl_q = 0.0
    for k in range(K):
        p, q, pool = ref[k] / P, gen[k] / Q, (ref[k] + gen[k]) / (P + Q)
        se = math.sqrt(pool * (1.0 - pool) * (1.0 / P + 1.0 / Q))
        zk = (p - q) / se if se > 0 else 0.0
        z.append(zk)
        if abs(zk) > z_threshold:
            ndb += 1
        m = 0.5 * (p + q)
        if p > 0:
            kl_p += p * math.log2(p / m)
        if q > 0:
            kl_q += q * math.log2(q / m)
    jsd = 0.5 * kl_p + 0.5 * kl_q
    return {'ndb': ndb, 'ndb_over_k': ndb / K, 'jsd': jsd, 'z': z}
