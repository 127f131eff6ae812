"""Tensor-level wrappers of the k-means kernels (include/pggan_hip_cluster.h, csrc/cluster.hip): the assignment, the per-bin sums and the
centroid update of ``metrics.NDB``.

PyTorch is the allocator and the stream provider, as in ops.py; here it also does the plumbing between the two passes over the stack --
a stable sort of the labels and a bincount, [M] integers -- which the C header leaves to the caller.  Integer arithmetic throughout: the
results are exact and the same from run to run.  No CPU fallback (``metrics.NDB(device='cpu')`` is a numpy twin of its own)."""
import torch

from . import _lib, ops
from .ops import _dev_tensor, _image_bytes, _stream, _u8_images, require_gpu

_C = _lib.CLUSTER_CONSTANTS          # every #define PG_* that include/pggan_hip_cluster.h carries

MAX_IMAGES = _C['PG_CLUSTER_MAX_IMAGES']                       # images of one fit: an int32 sum of that many bytes cannot overflow
MAX_BINS = ops.NN_MAX_QUERIES                                   # centroids are the queries of one pass of ops.l2dist_u8


def _bins(K, what):
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= MAX_BINS:
        raise ValueError('%s: K = %r (1 <= K <= %d)' % (what, K, MAX_BINS))
    return int(K)


def assign_u8(stack_u8, centroids_u8):
    """``stack_u8`` [M,C,r,r], ``centroids_u8`` [K,C,r,r] uint8 device images -> ``(label int32 [M], sqdist int64 [M])``: the nearest
    centroid of every image by exact squared L2 distance, the lower k of equal distances (``ops.l2dist_u8`` with the centroids as the
    queries, then pg_cluster_argmin_i64).  The stack may be a batch of generated images.  1 <= K <= ``MAX_BINS``.  No host
    synchronisation."""
    _u8_images(stack_u8, 'assign_u8 stack')
    _u8_images(centroids_u8, 'assign_u8 centroids')
    M, K = stack_u8.shape[0], _bins(centroids_u8.shape[0], 'assign_u8')
    dist = ops.l2dist_u8(stack_u8, centroids_u8)                # (checks the devices, the shapes and D % 16)
    label = torch.empty((M,), device=stack_u8.device, dtype=torch.int32)
    best = torch.empty((M,), device=stack_u8.device, dtype=torch.int64)
    _lib.call('pg_cluster_argmin_i64', dist.data_ptr(), K, M, label.data_ptr(), best.data_ptr(), _stream())
    return label, best


def cluster_sums_u8(stack_u8, label, K):
    """Per-bin sums of the images' bytes: ``stack_u8`` [M,C,r,r] uint8, ``label`` [M] int32 on the same device with values in
    -1 .. K-1 (-1: not a member, e.g. a held-out image -- it is not read) -> ``(sums int32 [K,C,r,r], counts int64 [K])``
    (pg_cluster_sums_u8).  The member list the kernel reads (image indices grouped by bin, a stable sort of the labels) and its
    offsets (a bincount) are made with torch's device ops.  1 <= M <= ``MAX_IMAGES``; a label outside -1 .. K-1 is a ValueError
    (one 1-element host read)."""
    _u8_images(stack_u8, 'cluster_sums_u8 stack')
    K = _bins(K, 'cluster_sums_u8')
    if stack_u8.shape[0] > MAX_IMAGES:
        raise ValueError('cluster_sums_u8: %d images (at most %d: the sums are int32)' % (stack_u8.shape[0], MAX_IMAGES))
    M, D = _image_bytes(stack_u8, 'cluster_sums_u8')
    _dev_tensor(label, torch.int32, (M,), stack_u8.device, 'cluster_sums_u8: label')
    require_gpu()
    if bool(((label < -1) | (label >= K)).any()):
        raise ValueError('cluster_sums_u8: labels must lie in -1 .. %d' % (K - 1))
    key = label.to(torch.int64) + 1                             # 0: not a member, 1 + k: bin k
    _, order = torch.sort(key, stable=True)                     # the non-members first, then bin after bin, images ascending
    offsets = torch.cumsum(torch.bincount(key, minlength=K + 1), 0)          # offsets[k] = non-members + members of the bins below k
    counts = offsets[1:] - offsets[:-1]
    order, offsets = order.to(torch.int32), offsets.to(torch.int32)
    sums = torch.empty((K,) + tuple(stack_u8.shape[1:]), device=stack_u8.device, dtype=torch.int32)
    _lib.call('pg_cluster_sums_u8', stack_u8.data_ptr(), M, D, order.data_ptr(), M, offsets.data_ptr(), K, sums.data_ptr(), _stream())
    return sums, counts


def centroids_u8(sums, counts, previous):
    """The centroid update: ``sums`` int32 [K,C,r,r] and ``counts`` int64 [K] of ``cluster_sums_u8``, ``previous`` uint8 [K,C,r,r] ->
    new uint8 [K,C,r,r]: ``(2 sums + n) // (2 n)``, the mean rounded half up, in 64-bit integers; a bin with n = 0 keeps its previous
    centroid (pg_cluster_centroids_u8, which updates the copy of ``previous`` made here in place)."""
    _u8_images(previous, 'centroids_u8 previous')
    K = _bins(previous.shape[0], 'centroids_u8')
    _, D = _image_bytes(previous, 'centroids_u8')
    _dev_tensor(sums, torch.int32, previous.shape, previous.device, 'centroids_u8: sums')
    _dev_tensor(counts, torch.int64, (K,), previous.device, 'centroids_u8: counts')
    require_gpu()
    out = torch.empty_like(previous)
    out.copy_(previous)
    _lib.call('pg_cluster_centroids_u8', sums.data_ptr(), counts.data_ptr(), out.data_ptr(), K, D, _stream())
    return out
