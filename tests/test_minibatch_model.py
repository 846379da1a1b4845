"""tests/minibatch_model.py against answers worked out by hand: the shuffle's permutation pi for V = 1, 2, 3 and 5 under one seed,
round by round; a 2 x 3 ring with two unclean transitions through index -> order -> a minibatch of 4 with its -1 slots; pi as a
bijection for every V in 1 .. 2100 and around the powers of two; two seeds, two orders; the float32 normalisation; the statistics."""
import math

import numpy as np

import minibatch_model as mm

SEED = 0x0123456789ABCDEF  # seed_lo 0x89ABCDEF, seed_hi 0x01234567
KEYS = [0x4C843A19, 0x09BBC2CF, 0xDA36C2A3, 0x5E3B515F, 0x98F92075, 0x106103B5]


def test_fmix_and_the_keys_by_hand():
    """key[0] = fmix(seed_lo ^ 0) ^ seed_hi, every line of fmix written out:
         x            = 0x89ABCDEF
         x ^= x >> 16 -> 0x89AB4444          (0x89ABCDEF ^ 0x000089AB)
         x *= 0x85ebca6b (mod 2^32) -> 0xACDF306C
         x ^= x >> 13 -> 0xACDA5695
         x *= 0xc2b2ae35 (mod 2^32) -> 0x4DA732D9
         x ^= x >> 16 -> 0x4DA77F7E
         ^ seed_hi    -> 0x4C843A19"""
    x = 0x89ABCDEF
    x ^= x >> 16
    assert x == 0x89AB4444
    x = (x * 0x85EBCA6B) % 2 ** 32
    assert x == 0xACDF306C
    x ^= x >> 13
    assert x == 0xACDA5695
    x = (x * 0xC2B2AE35) % 2 ** 32
    assert x == 0x4DA732D9
    x ^= x >> 16
    assert x == 0x4DA77F7E and x ^ 0x01234567 == KEYS[0]
    assert mm.fmix(0x89ABCDEF) == 0x4DA77F7E and mm.fmix(0) == 0 and mm.fmix(1) == 0x514E28B7
    assert mm.split_seed(SEED) == (0x89ABCDEF, 0x01234567)
    assert mm.keys(0x89ABCDEF, 0x01234567) == KEYS


def test_pi_by_hand_for_v_1_2_3_and_5():
    """V = 5: b = 3, hb = 1, ha = 2, mA = 3, mB = 1.  x = 0: L = 0, R = 0; the six rounds, with f = fmix(other half + key[r]):
         r0 f = 0xBEC153AD, L ^= f & 3 -> 1      r1 f = 0x2DFD7067, R ^= f & 1 -> 1      r2 f = 0x2BDEE78F, L -> 2
         r3 f = 0xF5D5B4A4, R -> 1               r4 f = 0x0D636E11, L -> 3               r5 f = 0xDD22EFF9, R -> 0
       x = (3 << 1) | 0 = 6 >= 5: once more from 6 (L = 3, R = 0):
         r0 0xBEC153AD L -> 2   r1 0x3082E8BD R -> 1   r2 0x2BDEE78F L -> 1   r3 0x00D88DC0 R -> 1   r4 0x0D636E11 L -> 0   r5 0xC15087C8 R -> 1
       x = 1.  So pi(0) = 1 after two passes; likewise 2 -> 7 -> 4, and 1 -> 3, 3 -> 2, 4 -> 0 in one pass.
       V = 3: b = 2, hb = ha = 1.  x = 0: r0 L -> 1, r1 (0x2DFD7067) R -> 1, r2 L -> 0, r3 (0xECEF6949) R -> 0, r4 (0x912522F5) L -> 1,
       r5 (0x7A30B67A) R -> 0: x = 2.  V = 2: b = max(2, 1) = 2, so the walk runs over [0, 4) as well."""
    key = mm.keys(*mm.split_seed(SEED))
    f = [mm.fmix((0 + key[0]) % 2 ** 32), mm.fmix((1 + key[1]) % 2 ** 32), mm.fmix((1 + key[2]) % 2 ** 32)]
    assert f == [0xBEC153AD, 0x2DFD7067, 0x2BDEE78F]  # the first three rounds of V = 5, x = 0 above
    passes = [0]
    assert mm.perm(5, 0, key, passes) == 1 and passes == [2]
    assert [mm.perm(1, x, key) for x in range(1)] == [0]
    assert [mm.perm(2, x, key) for x in range(2)] == [0, 1]
    assert [mm.perm(3, x, key) for x in range(3)] == [2, 1, 0]
    assert [mm.perm(5, x, key) for x in range(5)] == [1, 3, 4, 2, 0]
    for V in (1, 2, 3, 5):
        assert mm.perm_all(V, key).tolist() == [mm.perm(V, x, key) for x in range(V)]
    assert mm.perm_all(0, key).tolist() == []


def test_a_2_by_3_ring_by_hand():
    """T = 2, R = 3, n = 2.  is_clean = [[1, 0, 1], [1, 1, 0]]: k = 1 and k = 5 do not count, valid = [0, 2, 3, 4], V = 4.
    pi over V = 4 under SEED is [2, 1, 3, 0], so order = [valid[2], valid[1], valid[3], valid[0], -1, -1] = [3, 2, 4, 0, -1, -1].
    Minibatch 0 of 4 takes k = 3, 2, 4, 0; minibatch 1 takes order[4], order[5] = -1, -1 and two positions past T R: four empty slots."""
    clean = np.array([[1, 0, 1], [1, 1, 0]], np.uint8)
    valid = mm.valid_list(clean, 2)
    assert valid.tolist() == [0, 2, 3, 4]
    assert mm.valid_list(clean, 1).tolist() == [0, 2]  # (the cursor cuts the list)
    key = mm.keys(*mm.split_seed(SEED))
    assert mm.perm_all(4, key).tolist() == [2, 1, 3, 0]
    order = mm.order_list(valid, 6, SEED)
    assert order.tolist() == [3, 2, 4, 0, -1, -1]
    obs = np.arange(3 * 3 * 2, dtype=np.uint8).reshape(3, 3, 2) + 1  # slot s, row r: bytes 6 s + 2 r + 1, + 2
    ring = {"actions": np.arange(18, dtype=np.float32).reshape(2, 3, 3), "rewards": np.array([[10, 11, 12], [13, 14, 15]], np.float32),
            "dones": np.array([[0, 0, 1], [1, 0, 0]], np.uint8), "dones_info": np.array([[0, 0, 5], [10, 0, 0]], np.int32)}
    adv = np.array([[0.5, 9, 1.5], [2.5, 3.5, 9]], np.float32)
    values = np.arange(9, dtype=np.float32).reshape(3, 3)  # [T + 1, R]: the same k
    mb = mm.gather(order, 0, 4, {"o": obs}, ring, [adv, values], 0, np.array([0.5, 2.0], np.float32))
    assert mb["mb_index"].tolist() == [3, 2, 4, 0] and mb["mb_weight"].tolist() == [1, 1, 1, 1]
    assert mb["mb_o"].tolist() == [[7, 8], [5, 6], [9, 10], [1, 2]]
    assert mb["mb_rewards"].tolist() == [13, 12, 14, 10] and mb["mb_dones"].tolist() == [1, 1, 0, 0] and mb["mb_dones_info"].tolist() == [10, 5, 0, 0]
    assert mb["mb_actions"].tolist() == [[9, 10, 11], [6, 7, 8], [12, 13, 14], [0, 1, 2]]
    assert mb["mb_scalars"].tolist() == [[4, 2, 6, 0], [3, 2, 4, 0]]  # (adv - 0.5) * 2; values as they are
    last = mm.gather(order, 1, 4, {"o": obs}, ring, [adv, values], 0, np.array([0.5, 2.0], np.float32))
    assert last["mb_index"].tolist() == [-1] * 4 and last["mb_weight"].tolist() == [0] * 4
    assert not last["mb_o"].any() and not last["mb_scalars"].any() and not last["mb_actions"].any() and not last["mb_rewards"].any()
    mixed = mm.gather(order, 1, 3, {"o": obs}, ring, [adv])  # slots 3, 4, 5 of the order
    assert mixed["mb_index"].tolist() == [0, -1, -1] and mixed["mb_weight"].tolist() == [1, 0, 0] and mixed["mb_scalars"].tolist() == [[0.5, 0, 0]]
    far = mm.gather(order, 100, 4, {"o": obs}, ring)  # j beyond the last minibatch
    assert far["mb_index"].tolist() == [-1] * 4 and far["mb_scalars"].shape == (0, 4)


def test_pi_is_a_bijection():
    longest = [0]
    for seed in (SEED, 0, 0xFFFFFFFFFFFFFFFF):
        key = mm.keys(*mm.split_seed(seed))
        for V in list(range(1, 2101)) + [4095, 4096, 4097, 65537]:
            p = mm.perm_all(V, key)
            assert p.dtype == np.uint32 and np.array_equal(np.sort(p), np.arange(V, dtype=np.uint32)), (seed, V)
        for V in (7, 100, 1025, 4097):  # the vectorised walk is the scalar one
            assert [mm.perm(V, x, key, longest) for x in range(0, V, 13)] == mm.perm_all(V, key)[::13].tolist()
    assert 1 <= longest[0] < 64


def test_two_seeds_two_orders():
    valid = np.arange(0, 600, 2, dtype=np.int32)
    a, b = mm.order_list(valid, 700, 1), mm.order_list(valid, 700, 2)
    assert (a != b).any() and sorted(a[:300].tolist()) == valid.tolist() == sorted(b[:300].tolist())
    assert (a[300:] == -1).all() and (b[300:] == -1).all()
    assert np.array_equal(a, mm.order_list(valid, 700, 1))
    assert (a[:300] != valid).any()  # (not the identity)
    assert (mm.order_list(valid, 700, 1 << 32) != a).any()  # seed_hi counts too
    assert mm.order_list(valid[:0], 5, 1).tolist() == [-1] * 5


def test_normalise_rounds_twice():
    x, norm = np.float32(1.0000001), np.array([1e-8, 3.0], np.float32)
    d = np.float32(x - norm[0])
    assert mm.normalise([x], norm)[0] == np.float32(d * norm[1])
    assert mm.normalise([0.75], [0.25, 2.0]).tolist() == [1.0]


def test_statistics():
    rng = np.random.default_rng(0)
    x = (1.0 + rng.standard_normal((5, 2000))).astype(np.float32)
    valid = np.flatnonzero(rng.random(10000) < 0.8).astype(np.int32)
    got = mm.stats(x, valid, 10000, 1e-8)
    assert got.tobytes() == mm.stats(x, valid, 10000, 1e-8).tobytes()
    v = x.reshape(-1)[valid].astype(np.float64)
    mean = math.fsum(v) / len(v)
    var = math.fsum((v - mean) ** 2) / len(v)  # the population variance
    assert got[0] == np.float32(mean)
    assert abs(float(got[1]) - 1.0 / math.sqrt(var + 1e-8)) <= np.spacing(np.float32(1.0 / math.sqrt(var + 1e-8)))
    assert abs(float(got[1]) - 1.0 / float(np.std(v, ddof=1))) > abs(float(got[1]) - 1.0 / float(np.std(v)))  # not torch's unbiased default
    assert mm.stats(x, valid[:0], 10000, 1e-8).tolist() == [0.0, 1.0]
    assert mm.stats(np.full((5, 2000), 3.0, np.float32), valid, 10000, 0.0).tolist() == [3.0, 1.0]  # var + eps == 0
    assert mm.fold(np.arange(256)) == 255 * 128
