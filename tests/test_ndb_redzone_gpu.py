"""The k-means kernels between guard bands (tests/redzone.py, docs/experiments_redzone.md): pg_cluster_argmin_i64, pg_cluster_sums_u8 and
pg_cluster_centroids_u8 read nothing outside their inputs, write no input, write nothing outside their outputs and leave no output
element unwritten.  The stack, the centroids, the labels, the member list and its offsets are guarded inputs; the outputs the wrappers
make themselves are guarded through ``AllocatorProxy`` on cluster.py's and ops.py's ``torch``.  D = 16 and 48 are the sizes where a 16-byte
load has no slack (one piece, and three pieces with a thread of the workgroup left over), 3x64x64 the one with slices; the image counts
end on the payload's last byte.  The uint8 output (the centroids) is run with both sentinels; the integer outputs cannot hold the
sentinel 0xA5A5.. (negative) by construction."""
import numpy as np
import pytest
import torch

import ndb_ref
from redzone import Redzone

import pggan_amd as pg

pytestmark = pytest.mark.gpu
cluster, ops = pg.cluster, pg.ops


@pytest.fixture
def rz(monkeypatch):
    r = Redzone('cuda')
    proxy = r.proxy(helpers=(ops._empty, ops.Arena.take))
    monkeypatch.setattr(ops, 'torch', proxy)
    monkeypatch.setattr(cluster, 'torch', proxy)
    yield r
    r.forget()


def chk(rz, **kw):
    try:
        rz.check(**kw)
    except RuntimeError as e:                                  # a device fault: nothing more is launched on it in this session
        pytest.exit('device error under the guard bands: %s' % (e,), returncode=3)


def images(n, C, r, seed):
    x = np.random.RandomState(seed).randint(0, 256, size=(n, C, r, r)).astype(np.uint8)
    x[x == 0xA5] = 0xA4
    x[x == 0x5A] = 0x5B
    return x


@pytest.mark.parametrize('M,K,C,r', [(37, 3, 1, 4), (130, 50, 3, 4), (257, 64, 3, 4), (5, 2, 3, 64)])
def test_assign_inside_guard_bands(rz, M, K, C, r):
    stack, cents = images(M, C, r, seed=41), images(K, C, r, seed=42)
    stack_d, cents_d = rz.guard(torch.from_numpy(stack), name='stack'), rz.guard(torch.from_numpy(cents), name='centroids')
    assert stack_d.data_ptr() % 32 == 16
    label, best = cluster.assign_u8(stack_d, cents_d)
    chk(rz)                                                    # dist, label, best: bands intact, every element written
    want_l, want_d = ndb_ref.assign(stack, cents)
    assert label.cpu().tolist() == want_l and best.cpu().tolist() == want_d


@pytest.mark.parametrize('M,K,C,r', [(37, 3, 1, 4), (300, 5, 3, 4), (5000, 1, 1, 4), (5, 2, 3, 64)])
def test_sums_inside_guard_bands(rz, M, K, C, r):
    """(5000 images in one bin of D = 16: the zeroing launch and the atomics.)  The last image of the stack is a member, so the last
    load ends on the payload's last byte; the wrapper's own output, then the C entry on a guarded member list and offsets."""
    stack = images(M, C, r, seed=43)
    labels = np.random.RandomState(44).randint(-1, K, size=M).astype(np.int32)
    labels[-1], labels[0] = K - 1, 0
    stack_d, label_d = rz.guard(torch.from_numpy(stack), name='stack'), rz.guard(torch.from_numpy(labels), name='label')
    sums, counts = cluster.cluster_sums_u8(stack_d, label_d, K)
    chk(rz)
    want_s, want_n = ndb_ref.sums(stack, labels.tolist(), K)
    assert counts.cpu().tolist() == want_n and np.array_equal(sums.cpu().numpy().astype(np.int64), want_s)
    order = np.argsort(labels, kind='stable').astype(np.int32)
    offsets = np.cumsum(np.bincount(labels + 1, minlength=K + 1)).astype(np.int32)
    order_d, off_d = rz.guard(torch.from_numpy(order), name='order'), rz.guard(torch.from_numpy(offsets), name='offsets')
    out = rz.out((K, C, r, r), torch.int32, name='sums')
    pg._lib.call('pg_cluster_sums_u8', stack_d.data_ptr(), M, C * r * r, order_d.data_ptr(), M, off_d.data_ptr(), K, out.data_ptr(),
                 ops._stream())
    chk(rz, keep_outputs=True)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), want_s)


@pytest.mark.parametrize('sentinel', [0, 1])
@pytest.mark.parametrize('K,C,r', [(3, 1, 4), (50, 3, 4), (2, 3, 64)])
def test_centroids_inside_guard_bands(rz, K, C, r, sentinel):
    rs = np.random.RandomState(45)
    counts = rs.randint(0, 4, size=K).astype(np.int64)
    counts[0], counts[-1] = 0, 3
    sums = images(K, C, r, seed=47).astype(np.int64) * counts[:, None, None, None]           # whole means: neither sentinel comes out
    sums[0] = 99                                               # count 0: not used
    previous = images(K, C, r, seed=46)
    want = ndb_ref.centroids(sums, counts.tolist(), previous)
    sums_d = rz.guard(torch.from_numpy(sums.astype(np.int32)), name='sums')
    counts_d, prev_d = rz.guard(torch.from_numpy(counts), name='counts'), rz.guard(torch.from_numpy(previous), name='previous')
    if sentinel == 0:
        got = cluster.centroids_u8(sums_d, counts_d, prev_d)   # the wrapper's copy of the previous centroids, updated in place
    else:
        got = rz.out((K, C, r, r), torch.uint8, name='centroids', sentinel=1)
        got.copy_(prev_d)
        pg._lib.call('pg_cluster_centroids_u8', sums_d.data_ptr(), counts_d.data_ptr(), got.data_ptr(), K, C * r * r, ops._stream())
    chk(rz)
    assert np.array_equal(got.cpu().numpy(), want)
