"""TEST INFRASTRUCTURE shared by tests/test_dataset_host.py, test_dataset_gpu.py and test_dataset_redzone_gpu.py: inputs with the
.5 ties of tests/golden/make_golden.py (make_io_steps) and the batch definition written with oracle/io_steps.py alone."""
import numpy as np

from oracle import io_steps as oio


def make_stack(M, C, S, seed=0):
    """uint8 [M,C,S,S]: uniform bytes with 0, 255, 1, 2, 254 at every 5th position -- block sums of 1, 2, 3 mod 4, i.e. the .5
    ties and the .25 / .75 cases of the rounded 2x2 mean, and both ends of the range."""
    x = np.random.RandomState(1000 * seed + 100 * C + S + M).randint(0, 256, size=(M, C, S, S)).astype(np.uint8)
    x.reshape(-1)[::5] = np.array([0, 255, 1, 2, 254], dtype=np.uint8)[np.arange(x.size)[::5] % 5]
    return x


def oracle_level(images, depthdiff, range_in=(0, 255)):
    if depthdiff == 0:
        return images
    return np.stack([oio.create_datapoint_from_depth(im, depthdiff, range_in) for im in images])


def oracle_batch(stack, idx, flip, depthdiff, alpha, range_in=(0, 255), range_out=(-1, 1)):
    """The batch by the oracle: level of image idx[j], np.flip of the LEVEL image where flagged, real_prepare."""
    level = oracle_level(stack[np.asarray(idx)], depthdiff, range_in)
    if flip is not None:
        level = np.stack([np.flip(im, -1) if f else im for im, f in zip(level, np.asarray(flip))])
    return oio.real_prepare(level, alpha, range_in, range_out)
