"""tests/ndb_ref.py, the CPU statement of NDB/k and JSD, against cases worked out by hand.  No GPU, no library."""
import math

import numpy as np

import ndb_ref


def test_two_bins_worked_by_hand():
    """ref = [30, 10] of P = 40, gen = [20, 20] of Q = 40: p = (3/4, 1/4), q = (1/2, 1/2), pool = (5/8, 3/8) in both bins' se."""
    res = ndb_ref.statistic([30, 10], [20, 20])
    se = math.sqrt((50 / 80) * (1.0 - 50 / 80) * (1.0 / 40 + 1.0 / 40))
    assert se == math.sqrt((30 / 80) * (1.0 - 30 / 80) * (1.0 / 40 + 1.0 / 40))          # 5/8 * 3/8 either way round
    assert res['z'] == [(0.75 - 0.5) / se, (0.25 - 0.5) / se]
    assert abs(res['z'][0] - 2.3094010767585034) < 1e-15                                 # 0.25 / sqrt(15/64 / 20) = sqrt(16/3)
    assert res['ndb'] == 2 and res['ndb_over_k'] == 1.0                                  # |z| = 2.309 > 1.96 in both
    m = (0.625, 0.375)
    kl_p = 0.75 * math.log2(0.75 / m[0]) + 0.25 * math.log2(0.25 / m[1])
    kl_q = 0.5 * math.log2(0.5 / m[0]) + 0.5 * math.log2(0.5 / m[1])
    assert res['jsd'] == 0.5 * kl_p + 0.5 * kl_q and 0.04 < res['jsd'] < 0.06            # 0.0488 bits
    # a looser threshold than |z|: nothing differs
    assert ndb_ref.statistic([30, 10], [20, 20], z_threshold=2.5)['ndb'] == 0


def test_equal_histograms_give_exactly_nothing():
    for ref in ([5, 5], [7, 0, 13, 1], [1] * 50, [3, 0, 0, 9]):
        res = ndb_ref.statistic(ref, list(ref))
        assert res['ndb'] == 0 and res['jsd'] == 0.0 and res['z'] == [0.0] * len(ref)
    # ... and proportions that are equal at different totals
    res = ndb_ref.statistic([10, 30], [5, 15])
    assert res['ndb'] == 0 and res['jsd'] == 0.0


def test_everything_generated_in_one_bin():
    """K equally filled bins, all Q = K n generated images in bin 0: every bin differs; JSD by its closed form, evaluated in the order
    the reference adds (bin 0 first): KL(p|m) = (1/K) log2((1/K) / m0) + (K - 1) (1/K) log2(2), KL(q|m) = log2(1 / m0), m0 = (1/K + 1) / 2."""
    for K, n in ((2, 100), (4, 100), (50, 40)):
        res = ndb_ref.statistic([n] * K, [K * n] + [0] * (K - 1))
        assert res['ndb'] == K and res['ndb_over_k'] == 1.0
        assert res['z'][0] < -1.96 and all(z > 1.96 for z in res['z'][1:])
        p, m0 = n / (K * n), 0.5 * (n / (K * n) + 1.0)
        kl_p = p * math.log2(p / m0)
        for _ in range(K - 1):
            kl_p += p * math.log2(p / (0.5 * (p + 0.0)))
        kl_q = 1.0 * math.log2(1.0 / m0)
        assert res['jsd'] == 0.5 * kl_p + 0.5 * kl_q
        assert 0.0 < res['jsd'] < 1.0
    # disjoint supports: the upper end of the range, exactly
    assert ndb_ref.statistic([8, 0], [0, 8])['jsd'] == 1.0


def test_a_bin_with_no_standard_error_is_not_different():
    """An empty bin in both histograms has pool = 0 and se = 0; a bin that holds EVERYTHING has pool = 1: z = 0 for both."""
    res = ndb_ref.statistic([10, 0, 30], [25, 0, 15])
    assert res['z'][1] == 0.0 and res['ndb'] == 2
    res = ndb_ref.statistic([40, 0], [40, 0])
    assert res['z'] == [0.0, 0.0] and res['ndb'] == 0 and res['jsd'] == 0.0


def test_assignment_update_and_rounding_by_hand():
    x = np.zeros((5, 1, 4, 4), dtype=np.uint8)
    x[0], x[1], x[2], x[3], x[4] = 0, 1, 2, 10, 13
    c = np.stack([x[0], x[3], x[3]])                                                     # two equal centroids
    labels, dists = ndb_ref.assign(x, c)
    assert labels == [0, 0, 0, 1, 1] and dists == [0, 16, 64, 0, 144]                    # the lower of the equal centroids wins; 2 is nearer 0
    s, n = ndb_ref.sums(x, [0, 0, -1, 1, 1], 3)                                          # image 2 held out
    assert n == [2, 2, 0] and s[0].reshape(-1).tolist() == [1] * 16 and s[1].reshape(-1).tolist() == [23] * 16
    new = ndb_ref.centroids(s, n, c)
    assert new[0].reshape(-1).tolist() == [1] * 16                                       # 0.5 rounds UP
    assert new[1].reshape(-1).tolist() == [12] * 16                                      # 11.5 rounds up
    assert np.array_equal(new[2], c[2])                                                  # the empty bin keeps its centroid
    big = np.full((1, 1, 4, 4), 255 * 2 ** 23, dtype=np.int64)                            # 2 sums reaches 2^32
    assert ndb_ref.centroids(big, [2 ** 23], c[:1])[0].reshape(-1).tolist() == [255] * 16
