"""seq_model.py without a device: the coverage the program generator promises over seeds
0..N_PROGRAMS-1, and the model against the oracle where the two can be compared directly."""
import numpy as np
import pytest

import seq_model as sm
from arena import CANARY


@pytest.fixture(scope="module")
def programs():
    return [sm.program(seed) for seed in range(sm.N_PROGRAMS)]


def library_calls(steps):
    return [st for st in steps if st.kind not in sm.TORCH_ONLY]


def pair_matrix(programs):
    """How often each ordered pair of distinct workspace users occurs as consecutive library calls."""
    count = {(u, v): 0 for u in sm.USERS for v in sm.USERS if u != v}
    for _, steps, _ in programs:
        calls = [sm.user_of(st) for st in library_calls(steps)]
        for u, v in zip(calls, calls[1:]):
            if u and v and u != v:
                count[(u, v)] += 1
    return count


def test_programs_are_well_formed(programs):
    for seed, (live, steps, ends_clean) in enumerate(programs):
        assert len(live) == 3 and len(set(live)) == 3 and set(live) <= set(sm.POOL), seed
        assert 12 <= len(steps) <= 16, (seed, len(steps))
        assert all(st.kind in sm.KINDS and (st.batch is None or st.batch in live) for st in steps), seed
        assert sm.program(seed)[1] == steps, "the generator is a function of the seed"
        for b in live:       # a heal follows its locate, nothing of the batch in between
            mine = [st.kind for st in steps if st.batch == b]
            for i, kd in enumerate(mine):
                if kd == "heal":
                    assert mine[i - 1] in ("locate", "locate_multi"), (seed, b, mine)
                if kd in ("locate", "locate_multi"):
                    assert mine[i - 1] in ("corrupt", "locate_multi"), (seed, b, mine)


def test_every_ordered_pair_of_workspace_users_is_adjacent(programs):
    count = pair_matrix(programs)
    print("ordered pairs of workspace users (row then column):")
    print("%8s" % "" + "".join("%8s" % v for v in sm.USERS))
    for u in sm.USERS:
        print("%8s" % u + "".join("%8s" % ("-" if u == v else count[(u, v)]) for v in sm.USERS))
    missing = [p for p, c in count.items() if c == 0]
    assert not missing, missing


def test_every_step_kind_occurs(programs):
    count = {kd: 0 for kd in sm.KINDS}
    for _, steps, _ in programs:
        for st in steps:
            count[st.kind] += 1
    assert min(count.values()) >= 5, count


def test_programs_that_grow_the_workspace_with_work_in_flight(programs):
    """A first workspace user on the small batch and a later one on a large batch; and, by the record
    layouts, the later call does ask for more bytes than every call before it: grow_plans drains the
    stream, frees and reallocates with the program's earlier calls queued."""
    assert sm.plan_bytes(sm.Step("reconstruct", "D", {})) == 67 * 32      # RS(6,9) block-order records
    assert sm.plan_bytes(sm.Step("recover", "A", dict(slots=4))) == 257 * 64
    assert sm.plan_bytes(sm.Step("reconstruct", "C", {})) == 131 * 160
    assert sm.plan_bytes(sm.Step("reconstruct_wide", "F", {})) == 37 * 736
    assert sm.plan_bytes(sm.Step("locate_multi", "A", {})) == 77 * 32 + 2064    # 257 x 2 words, to 16 bytes
    n = 0
    for _, steps, _ in programs:
        users = [st for st in steps if sm.user_of(st)]
        if users[0].batch in sm.SMALL_PLANS and any(st.batch in sm.LARGE_PLANS for st in users[1:]):
            assert library_calls(steps)[0] is not users[0], "other calls are queued before the first user"
            need = [sm.plan_bytes(st) for st in users]
            assert need[0] > 0 and any(b > max(need[:i]) for i, b in enumerate(need) if i), need
            n += 1
    assert n >= 4, n


def test_programs_that_meet_a_new_code_with_work_in_flight(programs):
    n = 0
    for _, steps, _ in programs:
        codes = [(sm.POOL[st.batch].k, sm.POOL[st.batch].m, sm.POOL[st.batch].kind == "xor")
                 for st in library_calls(steps) if st.batch]
        n += len(set(codes)) > 1 and codes[0] != codes[-1]
    assert n >= 4, n


def test_programs_with_failing_blocks_then_clean_steps(oracle, programs):
    n = with_sync = 0
    for seed in range(sm.N_PROGRAMS):
        t = sm.Trace(oracle, seed)
        bad = [i for i, c in enumerate(t.codes) if c != sm.OK]
        if bad and any(c == sm.OK and st.kind not in sm.TORCH_ONLY
                       for st, c in zip(t.steps[bad[0] + 1:], t.codes[bad[0] + 1:])):
            n += 1
            with_sync += any(st.kind == "sync" for st in t.steps[bad[0] + 1:])
            assert any(c != sm.OK for c in t.sync_codes)
    assert n >= 6 and with_sync >= 1, (n, with_sync)


SEEDS = [0, 1, 7, 13, 22, 30]


@pytest.fixture(scope="module", params=SEEDS)
def trace(request, oracle):
    return sm.Trace(oracle, request.param)


def test_clean_batches_hold_their_truth(oracle, trace):
    """A batch whose episodes all ended holds, below every block's length, its first data with the columns
    that update steps named replaced by the new arena's, and the oracle's parity of that data."""
    for b in trace.ends_clean:
        x, first = trace.batches[b], trace.initial[b]
        k = x.s.k
        want = x.dview(first["img"]).copy()
        new0 = x.dview(first["new"])
        times = np.zeros((x.s.B, k), dtype=int)
        for st, inp in zip(trace.steps, trace.inputs):
            if st.batch == b and st.kind == "update":
                col = sm.words_to_bits(inp["col"].reshape(x.s.B, x.Wk), k)
                times += col
                flip = np.where(times % 2 == 0, sm.NEW_FLIP, 0).astype(np.uint8)[:, :, None]
                want = np.where(col[:, :, None], new0 ^ flip, want)
        body = np.broadcast_to(x.body, want.shape)
        assert np.array_equal(x.dview(x.img)[body], want[body]), (trace.seed, b)
        par = x.encode_of(want)
        pbody = np.broadcast_to(x.body, par.shape)
        assert np.array_equal(x.pview(x.img)[pbody], par[pbody]), (trace.seed, b)
        # past the length a slot holds canary, or the zero fill of an output
        past = x.dview(x.img)[np.broadcast_to(x.pad, want.shape)]
        assert ((past == CANARY) | (past == 0)).all()
        assert (x.dview(x.img)[np.broadcast_to(~x.body & ~x.pad, want.shape)] == CANARY).all()


def test_verify_reports_the_blocks_a_step_touched(oracle):
    for bid in "ADF":
        x = sm.Batch(sm.POOL[bid], oracle, 5)
        x.verify({})
        assert (x.w("status") == 1).all() and x.w("counts")[0] == 0 and x.w("counts")[1] == sm.STALE
        x.corrupt(dict(seed=3, t=1))
        touched = np.array([bool(h) for h in x.hit])
        assert touched.any() and not touched.all()
        x.verify({})
        assert np.array_equal(x.w("status") == 0, touched) and x.w("counts")[0] == touched.sum()
        y = sm.Batch(sm.POOL[bid], oracle, 5)
        y.erase(dict(seed=4, mode="any"))
        y.verify({})
        lost_below_l = (~y.present).any(axis=1)
        assert np.array_equal(y.w("status") == 0, lost_below_l) and y.w("counts")[0] == lost_below_l.sum()


def test_update_model_equals_the_encode_of_the_merged_data(oracle):
    for bid in "ABEF":
        x = sm.Batch(sm.POOL[bid], oracle, 11)
        k = x.s.k
        old, new = x.dview(x.img).copy(), x.dview(x.new).copy()
        _, inp = x.update(dict(seed=17))
        col = sm.words_to_bits(inp["col"].reshape(x.s.B, x.Wk), k)
        assert col.any() and not col.all(axis=1).all()
        merged = np.where(col[:, :, None], new, old)
        assert np.array_equal(x.dview(x.img), merged)
        par = x.encode_of(merged)
        body = np.broadcast_to(x.body, par.shape)
        assert np.array_equal(x.pview(x.img)[body], par[body])
        touched = np.broadcast_to(col.any(axis=1)[:, None, None] & x.pad, par.shape)
        assert not x.pview(x.img)[touched].any() and (x.pview(x.img)[np.broadcast_to(
            ~col.any(axis=1)[:, None, None] & ~x.body, par.shape)] == CANARY).all()
        # encode-idx: folding every column into a zeroed parity is the encode
        z = sm.Batch(sm.POOL[bid], oracle, 11)
        z.pview(z.img)[...] = 0
        z.fold(np.ones((z.s.B, k), dtype=bool), z.dview(z.img))
        assert np.array_equal(z.pview(z.img)[body], z.encode_of(z.dview(z.img))[body])


def test_sticky_code_priority():
    S = sm.Step
    steps = [S("reconstruct", "A", {}), S("recover", "A", {}), S("sync", None, {}), S("ragged_encode", "H", {}),
             S("verify", "A", {})]
    assert sm.expected_codes(steps, [sm.INVALID, sm.TOO_FEW, 0, sm.SHARD_SIZE, 0]) == [sm.TOO_FEW, sm.SHARD_SIZE]
    assert sm.worst({sm.SHARD_SIZE, sm.INVALID}) == sm.INVALID and sm.worst(set()) == sm.OK
