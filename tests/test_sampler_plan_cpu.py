"""The sample stage's launch plan (`sample_plan`, impact_amd/csrc/sampler_host.hpp) through its developer export `ivx_sampler_plan`, on the host
alone: a numpy restatement of the launcher's rules — which evaluator classes run and how large, who hosts the presets, what becomes of a
pre-pass that ran ahead — compared word by word over the whole table of inputs, the plan's invariants, and the transitions of sample-ahead's
state (idle / wanted / pending)."""
import itertools

import numpy as np
import pytest

from impact_amd import capi

SUPER_MAX_WORDS = 64  # (sampler_host.hpp; test_the_super_block_threshold pins it)
N_CU = 256
FILL = 4 * 5 * N_CU  # list entries that fill the chip a few times over: below it the first two classes share a launch
EVAL, ALL_GROUPS = 4, 7  # IVX_SCRATCH_EVAL; regions | mesher | eval
IDLE, WANTED, PENDING = 0, 1, 2
IN_COLS = ["n_nodes", "stack", "noise", "resident", "valid", "l0", "l1", "l2", "n_chunks", "cx", "cy", "cz", "n_cu", "dirty", "presets", "on", "state", "later_on",
           "later_n"]
assert len(IN_COLS) == capi.SAMPLER_PLAN_IN_WORDS
LAUNCH_COLS = ["mode", "noise", "grid", "lds_bytes", "scratch_off", "list", "long_count", "first", "commits_shadow"]
HEAD_COLS = ["words", "fused_super", "sx", "sy", "sz", "consume", "cancel", "super_presets", "prepass_presets", "first_presets", "clear_counters", "ahead_wanted",
             "n_launches"]
TAIL = {"state_after": 43, "state_after_wish": 44, "wish_launches": 45, "state_after_cancel": 46, "cancel_waits": 47}


def run_plans(table):
    """ivx_sampler_plan over every row of `table` [n, 19]"""
    table = np.ascontiguousarray(table, dtype=np.uint32)
    out = np.full((table.shape[0], capi.SAMPLER_PLAN_OUT_WORDS), 0xDEADBEEF, np.uint32)
    fn, a, b = capi.lib().ivx_sampler_plan, table.ctypes.data, out.ctypes.data
    sa, sb = table.strides[0], out.strides[0]
    for i in range(table.shape[0]):
        rc = fn(a + i * sa, b + i * sb)
        assert rc == capi.IVX_OK, (rc, table[i])
    return out


def restate(table):
    """the rules of the launcher, whole columns at a time: the expected output words [n, 48]"""
    c = {k: table[:, i].astype(np.int64) for i, k in enumerate(IN_COLS)}
    b = {k: c[k] != 0 for k in ("noise", "resident", "valid", "dirty", "on", "later_on")}
    n = table.shape[0]
    out = np.zeros((n, capi.SAMPLER_PLAN_OUT_WORDS), np.int64)
    words = np.maximum((c["n_nodes"] + 31) // 32, 1)
    fused = words <= SUPER_MAX_WORDS
    known = b["resident"] & b["valid"]
    l0, l1, l2 = c["l0"], c["l1"], c["l2"]
    fill = 4 * 5 * c["n_cu"]
    noise = b["noise"]
    merge01 = ~noise & known & (l0 > 0) & (l1 > 0) & ((l0 < fill) | (l1 < fill))
    launch2 = ~noise & ~merge01 & ~(known & (l0 == 0))
    launch1 = ~noise & (merge01 | ~(known & (l1 == 0)))
    launch0 = (noise | (c["stack"] >= 3)) & ~(known & (l2 == 0))
    fits = b["resident"] & fused & (launch0 | launch1 | launch2)
    pending = b["resident"] & (c["state"] == PENDING)
    consume, cancel = pending & fits, pending & ~fits
    host = c["presets"] & ~EVAL
    super_p = np.where(fused, 0, c["presets"])
    clear = b["dirty"] & ((super_p & EVAL) == 0)
    super_p = np.where(b["dirty"], super_p, super_p & ~EVAL)
    head = [words, fused, (c["cx"] + 3) // 4, (c["cy"] + 3) // 4, (c["cz"] + 3) // 4, consume, cancel, np.where(consume, 0, super_p),
            np.where(consume, 0, np.where(fused, host, 0)), np.where(consume, host, 0), clear & ~consume, b["on"] & fits,
            launch2.astype(np.int64) + launch1 + launch0]
    for i, col in enumerate(head):
        out[:, i] = col
    cap = np.minimum(c["n_chunks"], 16384)

    def fit(length):
        each = np.maximum((length + cap - 1) // cap, 1)
        return np.where(~known | (length == 0), cap, (length + each - 1) // each)

    def put(rows, slot, **w):
        for k, v in w.items():
            col = 13 + 10 * slot[rows] + LAUNCH_COLS.index(k)
            out[np.nonzero(rows)[0], col] = (v[rows] if isinstance(v, np.ndarray) else v)
        out[np.nonzero(rows)[0], 13 + 10 * slot[rows] + LAUNCH_COLS.index("commits_shadow")] = (consume & (slot == 0))[rows]

    zero = np.zeros(n, np.int64)
    lv = np.maximum(c["stack"], 1)
    put(launch2, zero, mode=2, noise=0, grid=fit(l0), lds_bytes=(4096 + 64) * 4, scratch_off=4096, list=0, long_count=1, first=0)
    off1 = 4096 + 15 * 256
    put(launch1 & merge01, zero, mode=1, noise=0, grid=fit(l0 + l1), lds_bytes=(off1 + 64) * 4, scratch_off=off1, list=0, long_count=1, first=1)
    put(launch1 & ~merge01, launch2.astype(np.int64), mode=1, noise=0, grid=fit(l1), lds_bytes=(off1 + 64) * 4, scratch_off=off1, list=1, long_count=0, first=0)
    put(launch0, launch2.astype(np.int64) + launch1, mode=0, noise=noise.astype(np.int64), grid=fit(l2), lds_bytes=lv * 4096 * 4, scratch_off=lv * 4096 - 16, list=2,
        long_count=0, first=0)
    # sample-ahead's two flags of old: a pre-pass pending stays so through a stage that is not the resident program's; the wish is this stage's
    still_pending = (c["state"] == PENDING) & ~b["resident"]
    after = np.where(still_pending, PENDING, np.where(b["on"] & fits, WANTED, IDLE))
    out[:, TAIL["state_after"]] = after
    out[:, TAIL["wish_launches"]] = (after == WANTED) & b["later_on"] & (c["later_n"] > 0) & ((c["later_n"] + 31) // 32 <= SUPER_MAX_WORDS)
    out[:, TAIL["state_after_wish"]] = np.where(after == WANTED, IDLE, after)
    out[:, TAIL["state_after_cancel"]] = IDLE
    out[:, TAIL["cancel_waits"]] = c["state"] == PENDING
    return out.astype(np.uint32)


def full_table():
    lens = [(0, 0, 0, 0)] + [(1, a, b_, c_) for a, b_, c_ in itertools.product((0, 1, FILL - 1, FILL, 100000), repeat=3)]
    grids = [(1, 1, 1, 1), (512, 8, 8, 8), (16384, 32, 32, 16), (32768, 32, 32, 32)]
    axes = [
        [0, 1, 32, 33, 32 * SUPER_MAX_WORDS, 32 * SUPER_MAX_WORDS + 1],  # n_nodes
        [0, 1, 2, 3, 9],  # stack_size
        [0, 1],  # noise
        [0, 1],  # resident
        range(len(lens)),
        range(len(grids)),
        [0, 1],  # eval_dirty
        [0, ALL_GROUPS],  # preset_groups
        [(0, IDLE), (0, PENDING), (1, IDLE), (1, PENDING)],  # sample-ahead on, a pre-pass pending
    ]
    idx = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(len(a)) for a in axes], indexing="ij")], axis=1)
    col = lambda k, vals: np.asarray(vals, dtype=np.int64)[idx[:, k]]  # noqa: E731
    lens_a, grids_a, ahead_a = np.asarray(lens), np.asarray(grids), np.asarray(axes[8])
    t = np.zeros((idx.shape[0], len(IN_COLS)), np.int64)
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = col(0, axes[0]), col(1, axes[1]), col(2, axes[2]), col(3, axes[3])
    t[:, 4:8] = lens_a[idx[:, 4]]
    t[:, 8:12] = grids_a[idx[:, 5]]
    t[:, 12] = N_CU
    t[:, 13], t[:, 14] = col(6, axes[6]), col(7, axes[7])
    t[:, 15:17] = ahead_a[idx[:, 8]]
    t[:, 17], t[:, 18] = t[:, 15], t[:, 0]  # (the step that acts on the wish finds the setting and the program unchanged)
    return t.astype(np.uint32)


@pytest.fixture(scope="module")
def plans():
    table = full_table()
    return table, run_plans(table)


def test_every_combination_agrees_with_the_restatement(plans):
    table, got = plans
    assert table.shape[0] == 6 * 5 * 2 * 2 * 126 * 4 * 2 * 2 * 4
    want = restate(table)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad.size, dict(zip(IN_COLS, table[bad[0]])), np.nonzero(got[bad[0]] != want[bad[0]])[0], got[bad[0]], want[bad[0]])


def test_invariants(plans):
    table, got = plans
    c = {k: table[:, i] for i, k in enumerate(IN_COLS)}
    h = {k: got[:, i] for i, k in enumerate(HEAD_COLS)}
    L = [{k: got[:, 13 + 10 * s + i] for i, k in enumerate(LAUNCH_COLS)} for s in range(3)]
    n = h["n_launches"]
    assert n.max() == 3 and n.min() == 0  # (never more than three; none when every list is known to be empty)
    for s in range(3):  # nothing stands in the entries behind the last launch
        assert not got[:, 13 + 10 * s:23 + 10 * s][n <= s].any()
    merged = (n >= 1) & (L[0]["first"] == 1)
    assert merged.any() and np.all(L[0]["mode"][merged] == 1)  # merge01 excludes the one-level launch: the merged launch is the two-level kernel, first in line
    for s in range(3):
        live = n > s
        assert not np.any(live & (L[s]["mode"] == 2) & (s > 0))  # the one-level class is first or absent
        noisy = live & (c["noise"] != 0)
        assert np.all(L[s]["mode"][noisy] == 0) and np.all(L[s]["noise"][noisy] == 1)  # noise programs launch the general class only, in its noise form
        assert np.all(L[s]["noise"][live & (c["noise"] == 0)] == 0)
        assert np.all(L[s]["commits_shadow"][live] == ((h["consume"] == 1) & (s == 0))[live])  # on the first launch and on no other
        assert np.all(L[s]["lds_bytes"][live] <= 150 * 1024) and np.all(L[s]["grid"][live] >= 1) and np.all(L[s]["grid"][live] <= 16384)
    assert np.all(n[c["noise"] != 0] <= 1)
    consume = h["consume"] == 1
    assert consume.any() and np.all(h["fused_super"][consume] == 1) and np.all(n[consume] >= 1) and np.all(c["resident"][consume] == 1)
    assert not np.any(consume & (h["cancel"] == 1))
    assert np.all((consume | (h["cancel"] == 1)) == ((c["resident"] == 1) & (c["state"] == PENDING)))  # a pending pre-pass never outlives a resident stage
    assert not np.any(consume & ((h["super_presets"] | h["prepass_presets"] | h["clear_counters"]) != 0))  # no own pre-pass: nothing for it to host
    assert np.all((h["super_presets"] | h["prepass_presets"] | h["first_presets"])[c["presets"] == 0] == 0)
    assert np.all(h["ahead_wanted"] <= c["on"])


def plan_row(**kw):
    base = dict(n_nodes=5, stack=2, noise=0, resident=1, valid=0, l0=0, l1=0, l2=0, n_chunks=512, cx=8, cy=8, cz=8, n_cu=N_CU, dirty=1, presets=ALL_GROUPS, on=1,
                state=IDLE, later_on=1, later_n=5)
    assert set(kw) <= set(base)
    base.update(kw)
    return np.array([[base[k] for k in IN_COLS]], np.uint32)


def test_a_stack_beyond_the_lds_is_refused():
    out = np.zeros(capi.SAMPLER_PLAN_OUT_WORDS, np.uint32)
    for stack, rc in ((9, capi.IVX_OK), (10, capi.IVX_ERR_CAPACITY)):
        assert capi.lib().ivx_sampler_plan(plan_row(stack=stack).ctypes.data, out.ctypes.data) == rc
    assert b"forward stack of 10 blocks" in capi.lib().ivx_last_error()
    assert capi.lib().ivx_sampler_plan(None, out.ctypes.data) == capi.IVX_ERR_INVALID
    assert capi.lib().ivx_sampler_plan(plan_row(state=3).ctypes.data, out.ctypes.data) == capi.IVX_ERR_INVALID


def test_the_super_block_threshold():
    for n_nodes, fused in ((32 * SUPER_MAX_WORDS, 1), (32 * SUPER_MAX_WORDS + 1, 0)):
        out = run_plans(plan_row(n_nodes=n_nodes, later_n=n_nodes))[0]
        assert (out[0], out[1]) == ((n_nodes + 31) // 32, fused)
        assert out[11] == fused  # longer programs never want a pre-pass ahead


def test_sample_ahead_transitions():
    """every (state, event) pair: a stage under the resident program that fits / does not fit / another program's stage, the step acting on the
    wish under the same or a changed setting and program, a cancel"""
    long_n = 32 * SUPER_MAX_WORDS + 1
    rows, want = [], []
    for state in (IDLE, WANTED, PENDING):
        # a resident stage that can be consumed next time: consumes what is pending, wants the next
        rows.append(plan_row(state=state)), want.append(dict(consume=state == PENDING, cancel=0, state_after=WANTED, state_after_wish=IDLE, wish_launches=1))
        # ... with sample-ahead off by now: what is pending is still consumed, nothing more is wanted
        rows.append(plan_row(state=state, on=0, later_on=0)), want.append(dict(consume=state == PENDING, cancel=0, state_after=IDLE, state_after_wish=IDLE, wish_launches=0))
        # a resident stage under a program too long for the fused tables: cancels, wants nothing
        rows.append(plan_row(state=state, n_nodes=long_n, later_n=long_n)), want.append(dict(consume=0, cancel=state == PENDING, state_after=IDLE, wish_launches=0))
        # another program's stage (ivx_sdf_sample): leaves a pending pre-pass alone, drops a wish
        rows.append(plan_row(state=state, resident=0)), want.append(dict(consume=0, cancel=0, state_after=PENDING if state == PENDING else IDLE, wish_launches=0))
        # the wish is stale when the step acts on it: sample-ahead was turned off / a long program / no program came in between
        for later in (dict(later_on=0), dict(later_n=long_n), dict(later_n=0)):
            rows.append(plan_row(state=state, **later)), want.append(dict(state_after=WANTED, state_after_wish=IDLE, wish_launches=0))
        # a cancel forgets the wish as well as the pre-pass under way, and waits only for the latter
        rows.append(plan_row(state=state)), want.append(dict(state_after_cancel=IDLE, cancel_waits=state == PENDING))
    got = run_plans(np.concatenate(rows))
    np.testing.assert_array_equal(got, restate(np.concatenate(rows)))
    for i, w in enumerate(want):
        for k, v in w.items():
            col = TAIL[k] if k in TAIL else HEAD_COLS.index(k)
            assert got[i, col] == int(v), (i, k, rows[i], got[i])
