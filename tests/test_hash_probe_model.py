"""CPU replay of the insert protocol of the LDS hash set / map of
kernels_spgemm.hip (hset_insert, hmap_add), in the way
tests/test_classical_ref.py replays the device PMIS.

The model: the 64 lanes of a wave run the probe loop in lockstep. In one
iteration every active lane reads its slot; lanes that see their key are
done; lanes that see an empty slot try the compare-and-swap, one of them per
slot wins (the lowest or the highest lane, selectable) and is done, a loser
with the winner's key is done too, any other loser runs the loop again on the
same slot; lanes that see another key move to the next slot. A lane gives up,
and its key is dropped, when its budget reaches the table size. The budget
counts loop iterations ("iterations", the rule before the fix: a lost
compare-and-swap costs one unit) or slots moved past ("slots", the rule of
the kernels now).

Nothing here says what the hardware does under the old rule; the model's
arbitration is an assumption. What it proves is that under "slots" a row
that fits its table cannot lose a key, and that the inputs of
tests/test_gpu_sparse_products.py sit where "iterations" does."""

import numpy as np
import pytest

from tests.sparse_product_inputs import (SHORT_ROWS, arrival_schedule,
                                         tier_edge_case)

N_COLS = 8192 + 64


def hash_col(c):
    """hash_col of kernels_spgemm.hip on uint32 arrays."""
    a = np.atleast_1d(np.asarray(c)).astype(np.uint32)
    with np.errstate(over="ignore"):
        a = (a ^ np.uint32(61)) ^ (a >> np.uint32(16))
        a = a * np.uint32(9)
        a = a ^ (a >> np.uint32(4))
        a = a * np.uint32(0x27d4eb2d)
        a = a ^ (a >> np.uint32(15))
    return a


def replay_rows(schedules, cap, budget="slots", winner="lowest"):
    """Dropped keys of each row. schedules[r] is row r's arrival schedule: a
    list of steps, each an array of up to 64 keys (lane l carries key l)
    that enter the probe loop together. The rows are independent (one table
    each) and only batched for speed."""
    assert budget in ("iterations", "slots")
    assert winner in ("lowest", "highest")
    n_rows = len(schedules)
    n_steps = max([len(s) for s in schedules] + [0])
    keys_in = np.full((n_rows, n_steps, 64), -1, dtype=np.int64)
    for r, steps in enumerate(schedules):
        for s, keys in enumerate(steps):
            assert len(keys) <= 64
            keys_in[r, s, :len(keys)] = keys
    table = np.full(n_rows * cap, -1, dtype=np.int64)
    dropped = np.zeros(n_rows, dtype=np.int64)
    for s in range(n_steps):
        row, lane = np.nonzero(keys_in[:, s, :] >= 0)
        key = keys_in[row, s, lane]
        h = (hash_col(key) & np.uint32(cap - 1)).astype(np.int64)
        used = np.zeros(key.size, dtype=np.int64)
        while key.size:
            slot = row * cap + h
            k0 = table[slot]
            found = k0 == key
            empty = k0 == -1
            # compare-and-swap: one lane per empty slot wins
            e = np.flatnonzero(empty)
            order = e[np.lexsort((lane[e], slot[e]))]
            s_sorted = slot[order]
            first = np.ones(order.size, dtype=bool)
            if winner == "lowest":
                first[1:] = s_sorted[1:] != s_sorted[:-1]
            else:
                first[:-1] = s_sorted[1:] != s_sorted[:-1]
            table[s_sorted[first]] = key[order[first]]
            placed = empty & (table[slot] == key)   # won, or same key won
            lost = empty & ~placed
            occupied = ~found & ~empty
            h = np.where(occupied, (h + 1) & (cap - 1), h)
            used += occupied | (lost if budget == "iterations" else False)
            gave_up = (occupied | lost) & (used >= cap)
            np.add.at(dropped, row[gave_up], 1)
            keep = (occupied | lost) & ~gave_up
            row, lane, key, h, used = (row[keep], lane[keep], key[keep],
                                       h[keep], used[keep])
    return dropped


def dropped_keys(schedule, cap, budget="slots", winner="lowest"):
    """Number of keys one row with this arrival schedule loses."""
    return int(replay_rows([schedule], cap, budget, winner)[0])


def random_rows(rng, n_rows, width, per_step=64):
    """Rows of `width` random distinct columns arriving per_step at a time."""
    out = []
    for _ in range(n_rows):
        cols = rng.choice(N_COLS, size=width, replace=False)
        out.append([cols[t:t + per_step] for t in range(0, width, per_step)])
    return out


def test_hash_col_matches_the_kernel_arithmetic():
    def scalar(c):
        a = c & 0xffffffff
        a = ((a ^ 61) ^ (a >> 16)) & 0xffffffff
        a = (a * 9) & 0xffffffff
        a ^= a >> 4
        a = (a * 0x27d4eb2d) & 0xffffffff
        a ^= a >> 15
        return a
    cols = [0, 1, 61, 8255, 65536, 2 ** 31 - 1]
    assert hash_col(cols).tolist() == [scalar(c) for c in cols]


def test_replay_counts_an_overfull_row():
    """cap + 3 distinct keys: exactly 3 are dropped under either rule when
    they come one at a time."""
    rng = np.random.RandomState(0)
    for budget in ("iterations", "slots"):
        rows = random_rows(rng, 5, 64 + 3, per_step=1)
        assert replay_rows(rows, 64, budget).tolist() == [3] * 5


@pytest.mark.parametrize("winner", ["lowest", "highest"])
@pytest.mark.parametrize("cap,n_rows", [(64, 400), (512, 200)])
def test_slots_rule_never_drops_a_key_that_fits(cap, n_rows, winner):
    rng = np.random.RandomState(cap)
    for width in range(cap - 8, cap + 1):
        drops = replay_rows(random_rows(rng, n_rows, width), cap, "slots",
                            winner)
        assert not drops.any(), f"cap {cap} width {width}: {drops.sum()}"


@pytest.mark.parametrize("budget", ["iterations", "slots"])
def test_one_key_per_step_never_drops(budget):
    rng = np.random.RandomState(3)
    for width in range(56, 65):
        rows = random_rows(rng, 100, width, per_step=1)
        assert not replay_rows(rows, 64, budget).any()
    rows = random_rows(rng, 8, 512, per_step=1)
    assert not replay_rows(rows, 512, budget).any()


def test_duplicate_keys_of_one_step_share_a_slot():
    """mode 1 of the kernels: several lanes can carry one key in a step."""
    keys = np.array([5, 9, 5, 5, 9, 77])
    for winner in ("lowest", "highest"):
        assert dropped_keys([keys, keys[::-1]], 64, "slots", winner) == 0
        assert dropped_keys([keys], 64, "iterations", winner) == 0


@pytest.fixture(scope="module")
def edge():
    """The float64 / float32 input of the device tests."""
    return tier_edge_case(8192, short_rows=SHORT_ROWS)


def edge_schedules(edge, lo, hi):
    rows = np.flatnonzero(~edge.short & (edge.widths >= lo)
                          & (edge.widths <= hi))
    return [arrival_schedule(edge.A, edge.B, i) for i in rows]


@pytest.mark.parametrize("winner", ["lowest", "highest"])
def test_tier_edge_inputs_sit_where_the_old_rule_breaks(edge, winner):
    """The rows of the GPU tests that the 64-entry tier fills: the old rule
    drops keys among them, the new rule none."""
    rows = edge_schedules(edge, 1, 64)
    assert len(rows) >= 9 * 64
    old = replay_rows(rows, 64, "iterations", winner)
    print(f"{winner}: 'iterations' drops keys in {np.count_nonzero(old)} of "
          f"{len(rows)} rows of the 64-entry tier")
    assert old.sum() >= 1
    assert not replay_rows(rows, 64, "slots", winner).any()


def test_tier_edge_inputs_fit_the_512_tier_under_the_new_rule(edge):
    rows = edge_schedules(edge, 1, 512)
    assert not replay_rows(rows, 512, "slots").any()
    # a row one entry too wide does lose a key
    over = edge_schedules(edge, 513, 513)
    assert len(over) == 2 and (replay_rows(over, 512, "slots") >= 1).all()
