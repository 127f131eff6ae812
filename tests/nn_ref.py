"""TEST INFRASTRUCTURE: the nearest-neighbour search of csrc/nn_search.hip / metrics.NearestNeighbours stated in numpy int64 (DESIGN.md
section 7), written from the definition and not from the kernels.  Everything is exact integer arithmetic: the tests compare with ``==``."""
import numpy as np


def l2dist(stack, queries):
    """int64 [K,M]: sum_d (stack[m, d] - queries[k, d])^2 over the bytes of an image."""
    x = np.asarray(stack).reshape(len(stack), -1).astype(np.int64)
    q = np.asarray(queries).reshape(len(queries), -1).astype(np.int64)
    if x.size * len(q) <= 1 << 24:
        return ((x[None] - q[:, None]) ** 2).sum(-1)
    return np.stack([((x - qk[None]) ** 2).sum(-1) for qk in q])           # the same sums, one query at a time (memory)


def topk_smallest(dist, k):
    """(values [K,k], indices [K,k]) of the k smallest of every row, ascending by (value, index)."""
    dist = np.asarray(dist)
    order = np.stack([np.lexsort((np.arange(row.size), row))[:k] for row in dist])
    return np.take_along_axis(dist, order, axis=1), order.astype(np.int64)


def search(stack, queries, k):
    return topk_smallest(l2dist(stack, queries), k)


def search_mirror(stack, queries, k):
    """(sqdist, index, mirrored) [K,k] each: the k smallest keys (sqdist, index, mirrored) among the k nearest of every query and the
    k nearest of its left-right mirror image."""
    queries = np.asarray(queries)
    sq_a, ix_a = search(stack, queries, k)
    sq_b, ix_b = search(stack, queries[..., ::-1], k)
    sq, ix, mr = [], [], []
    for i in range(len(queries)):
        keys = sorted([(int(s), int(j), False) for s, j in zip(sq_a[i], ix_a[i])] + [(int(s), int(j), True) for s, j in zip(sq_b[i], ix_b[i])])[:k]
        sq.append([key[0] for key in keys])
        ix.append([key[1] for key in keys])
        mr.append([key[2] for key in keys])
    return np.array(sq, dtype=np.int64), np.array(ix, dtype=np.int64), np.array(mr, dtype=bool)


def images(n, C, r, seed):
    """uint8 [n,C,r,r]: random bytes with 0, 127, 128 and 255 forced into every image (both ends of the range and the two values either
    side of the shift by 128)."""
    x = np.random.RandomState(seed).randint(0, 256, size=(n, C * r * r)).astype(np.uint8)
    pos = np.random.RandomState(seed + 1).permutation(C * r * r)[:4]
    x[:, pos] = np.array([0, 127, 128, 255], dtype=np.uint8)
    return x.reshape(n, C, r, r)
