"""tests/seq_model.py against answers derived by hand: a 2-row ring with n = 5 transitions stored of T = 6 and L = 2, so the last
chunk has one step.  Row 1's chunk 0 is wholly unclean, row 0's chunk 1 has an unclean step inside, final_idx is set in mid-chunk
(t = 3, row 0) and at slot 0 (row 0)."""
import numpy as np

import minibatch_model as mm
import seq_model as sm

R, T, N, L = 2, 6, 5, 2
#                     row 0, row 1
IS_CLEAN = np.array([[1, 0],    # t = 0   chunk 0: q = 0 clean, q = 1 wholly unclean
                     [1, 0],    # t = 1
                     [0, 7],    # t = 2   chunk 1: q = 2 with an unclean step inside, q = 3 clean (any non-zero byte counts)
                     [1, 1],    # t = 3
                     [1, 0],    # t = 4   chunk 2, one step: q = 4 clean, q = 5 unclean
                     [1, 1]], np.uint8)  # t = 5: not stored (n = 5); must not make q = 5 count
FINAL_IDX = np.full((T + 1, R), -1, np.int32)
FINAL_IDX[0, 0] = 0   # a reset at n = 0: row 0's episode starts at slot 0
FINAL_IDX[3, 0] = 1   # a reset in mid-chunk: row 0's episode starts at t = 3, step l = 1 of q = 2


def ring():
    t, row = np.meshgrid(np.arange(T + 1), np.arange(R), indexing="ij")
    x = (100 * t + 10 * row)[..., None] + np.arange(2)
    fields = {"x": x.astype(np.int16)}
    r = {"actions": np.stack([t[:T], row[:T], t[:T] + row[:T]], -1).astype(np.float32), "rewards": (t[:T] - row[:T]).astype(np.float32),
         "dones": (t[:T] == 2).astype(np.uint8), "dones_info": (t[:T] * 2 + row[:T]).astype(np.int32)}
    scalar = (t + 0.5 * row).astype(np.float32)
    state = (1000 + t * R + row).astype(np.float32)[..., None]
    return fields, r, scalar, state


def test_chunks_and_flags():
    assert sm.chunks(N, L) == 3 and sm.chunks(T, L) == 3 and sm.chunks(6, 4) == 2 and sm.chunks(1, 4) == 1
    assert sm.flags(IS_CLEAN, N, L).tolist() == [1, 0, 1, 1, 1, 0]
    assert sm.flags(IS_CLEAN, 6, L).tolist() == [1, 0, 1, 1, 1, 1]  # with t = 5 stored, q = 5 counts
    assert sm.flags(IS_CLEAN, 2, L).tolist() == [1, 0]
    assert sm.valid_list(IS_CLEAN, N, L).tolist() == [0, 2, 3, 4]
    assert sm.valid_list(IS_CLEAN, N, L).dtype == np.int32
    assert sm.flags(IS_CLEAN, N, 1).tolist() == IS_CLEAN[:N].reshape(-1).astype(bool).astype(int).tolist()  # L = 1: the transitions
    assert sm.flags(IS_CLEAN, N, 6).tolist() == [1, 1]  # L = T: one chunk per row


def test_order_is_the_minibatches_permutation_over_the_sequences():
    valid = sm.valid_list(IS_CLEAN, N, L)
    seed = 0x0123456789ABCDEF
    order = sm.order_list(valid, 6, seed)
    key = mm.keys(*mm.split_seed(seed))
    assert order[:4].tolist() == [int(valid[mm.perm(4, p, key)]) for p in range(4)]
    assert sorted(order[:4].tolist()) == [0, 2, 3, 4] and order[4:].tolist() == [-1, -1]
    assert sm.order_list(valid[:0], 6, seed).tolist() == [-1] * 6


def test_gather_by_hand():
    fields, r, scalar, state = ring()
    order = np.array([3, 0, 4, 2, -1, -1], np.int32)
    norm = np.array([1.0, 2.0], np.float32)

    def mb(j):
        return sm.gather(order, j, 3, L, N, R, fields, r, IS_CLEAN, FINAL_IDX, [scalar], 0, norm, [state])
    a = mb(0)  # slots q = 3 (c 1, row 1: t 2, 3), q = 0 (c 0, row 0: t 0, 1), q = 4 (c 2, row 0: t 4, and t 5 is not stored)
    assert a["mb_seq"].tolist() == [3, 0, 4] and a["mb_seq_len"].tolist() == [2, 2, 1]
    assert a["mb_index"].tolist() == [[5, 0, 8], [7, 2, -1]]
    assert a["mb_weight"].tolist() == [[1, 1, 1], [1, 1, 0]]
    assert a["mb_first"].tolist() == [[0, 1, 0], [0, 0, 0]]  # slot 0 of row 0
    assert a["mb_x"].tolist() == [[[210, 211], [0, 1], [400, 401]], [[310, 311], [100, 101], [0, 0]]]
    assert a["mb_x"].dtype == np.int16
    assert a["mb_actions"].tolist() == [[[2, 1, 3], [0, 0, 0], [4, 0, 4]], [[3, 1, 4], [1, 0, 1], [0, 0, 0]]]
    assert a["mb_rewards"].tolist() == [[1, 0, 4], [2, 1, 0]]
    assert a["mb_dones"].tolist() == [[1, 0, 0], [0, 0, 0]]
    assert a["mb_dones_info"].tolist() == [[5, 0, 8], [7, 2, 0]]
    assert a["mb_scalars"].tolist() == [[[3.0, -2.0, 6.0], [5.0, 0.0, 0.0]]]  # (t + row / 2 - 1) * 2; 0 where the step is missing
    assert a["mb_seq_state0"].view(np.float32).reshape(-1).tolist() == [1005, 1000, 1008]  # the FIRST step's row
    b = mb(1)  # q = 2 (c 1, row 0: t 2 unclean, t 3 behind a reset), then two slots behind the valid list
    assert b["mb_seq"].tolist() == [2, -1, -1] and b["mb_seq_len"].tolist() == [2, 0, 0]
    assert b["mb_index"].tolist() == [[4, -1, -1], [6, -1, -1]]
    assert b["mb_weight"].tolist() == [[0, 0, 0], [1, 0, 0]]  # the unclean step inside weighs nothing, but is there
    assert b["mb_first"].tolist() == [[0, 0, 0], [1, 0, 0]]   # the reset in mid-chunk
    assert b["mb_x"].tolist() == [[[200, 201], [0, 0], [0, 0]], [[300, 301], [0, 0], [0, 0]]]
    assert b["mb_scalars"].tolist() == [[[2.0, 0.0, 0.0], [4.0, 0.0, 0.0]]]
    assert b["mb_seq_state0"].view(np.float32).reshape(-1).tolist() == [1004, 0, 0]
    c = mb(2)  # beyond the last minibatch: positions 6 .. 8 >= C_max R
    assert c["mb_seq"].tolist() == [-1] * 3 and not c["mb_weight"].any() and not c["mb_x"].any() and (c["mb_index"] == -1).all()
    assert not c["mb_seq_state0"].any() and not c["mb_first"].any() and not c["mb_scalars"].any()


def test_gather_without_normalisation_and_two_states():
    fields, r, scalar, state = ring()
    order = np.array([4, -1, -1, -1, -1, -1], np.int32)
    wide = np.arange((T + 1) * R * 6, dtype=np.float32).reshape(T + 1, R, 6)
    m = sm.gather(order, 0, 2, L, N, R, fields, r, IS_CLEAN, FINAL_IDX, [scalar, scalar], None, None, [state, wide])
    assert m["mb_scalars"][:, :, 0].tolist() == [[4.0, 0.0], [4.0, 0.0]]
    assert m["mb_seq_state1"].shape == (2, 24) and m["mb_seq_state1"][0].view(np.float32).tolist() == wide[4, 0].tolist()
    assert not m["mb_seq_state1"][1].any()
