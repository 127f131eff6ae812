"""TEST INFRASTRUCTURE shared by tests/test_crops_host.py, test_crops_gpu.py and test_crops_redzone_gpu.py: strips with the .5 ties
of tests/dataset_ref.py and the materialised windows that define a crop batch."""
import numpy as np

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
