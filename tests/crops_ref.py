"""TEST INFRASTRUCTURE shared by tests/test_crops_host.py, test_crops_gpu.py and test_crops_redzone_gpu.py: strips with the .5 ties
of tests/dataset_ref.py and the materialised windows that define a crop batch; and the two identities the strip dataset shares with
the image dataset, stated once for host mode and for the device."""
import numpy as np
import torch

from dataset_ref import make_stack


def make_strips(C, R, widths=(1, 2, 3), extra=0, seed=0):
    """uint8 strips [C,R,w R + extra] (``make_stack`` bytes: ties, .25 / .75 cases, both ends of the range), one per width."""
    return [np.ascontiguousarray(make_stack(w * R + extra, C, R, seed=seed + k).transpose(1, 2, 0, 3).reshape(C, R, -1)[:, :, :w * R + extra])
            for k, w in enumerate(widths)]


def windows(strips, idx, starts, S):
    """uint8 [n,C,S,S]: columns [starts[j], starts[j] + S) of strip idx[j]."""
    out = [np.asarray(strips[m])[:, :, t:t + S] for m, t in zip(idx, starts)]
    assert all(w.shape[-1] == S for w in out)
    return np.stack(out)


def all_starts(strips, S):
    """Every legal (strip, start column): every residue mod 16 a strip has room for, and the last legal start of the last strip last."""
    idx = np.concatenate([np.full(s.shape[2] - S + 1, m, dtype=np.int64) for m, s in enumerate(strips)])
    u = np.concatenate([np.arange(s.shape[2] - S + 1, dtype=np.int64) for s in strips])
    return idx, u


def pyramid(strips, k, level_host):
    """The strips k levels down by repeated ``level_host(., 1)``."""
    for _ in range(k):
        strips = [level_host(s, 1) for s in strips]
    return strips


def check_square_strips_equal_the_stack(pg, C, R, pyr, device, M=5):
    """M images [C,R,R] as a stack and as M square strips, unshuffled: the two datasets are the same dataset.  The image stream takes
    its mirror flags from a generator seeded seed + 1, the crop stream from seed + 2: 8 and 7 meet at 9."""
    stack = make_stack(M, C, R, seed=C + R)
    kw = dict(pyramid=pyr, shuffle=False, mirror_augment=True, alpha=0.3, device=device)
    a = pg.DeviceImageDataset(stack, seed=8, two_channel=C == 2, **kw)
    b = pg.DeviceStripDataset(list(stack), seed=7, **kw)
    assert a.shape == b.shape == (M, C, R, R) and len(a) == len(b) == M
    for depth in range(R.bit_length() - 2):                                           # 4x4 .. R x R
        a.model_depth = b.model_depth = depth
        for n in (3, 4):                                                              # 7 of M = 5: every stage crosses an epoch boundary
            x, y = a.batch(n), b.batch(n)
            assert x.dtype == torch.float32 and tuple(x.shape) == (n, C, 4 << depth, 4 << depth) and x.device.type == torch.device(device).type
            assert torch.equal(x, y)
        assert torch.equal(a.level_stack(), b.level_stack())
        assert torch.equal(a[M - 1], b[M - 1])
        assert a.cursor == b.cursor == 7 * (depth + 1)


def check_items(ds, depths):
    """``ds.items(idx)`` of the last three items is the stack of ``ds[i]``: with alpha 1 whatever ``ds.alpha`` says, with the alpha
    given; the training cursor stays."""
    ds.batch(2)
    cursor = ds.cursor
    idx = torch.arange(len(ds) - 3, len(ds), dtype=torch.int64, device=ds.device)
    for depth in depths:
        ds.model_depth = depth
        for alpha in (1.0, 0.4):
            ds.alpha = alpha
            want = torch.stack([ds[i] for i in idx.tolist()])
            ds.alpha = 0.7
            got = ds.items(idx) if alpha == 1.0 else ds.items(idx, alpha=alpha)
            assert got.dtype == torch.float32 and got.device.type == ds.device.type and torch.equal(got.cpu(), want)
    assert ds.cursor == cursor
    return idx
