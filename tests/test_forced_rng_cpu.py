"""The RNG restatement's rare branches, forced on purpose (CPU part): the forcing helper against numpy, the oracle's generator primitives
against numpy's Generator at forced states, and the oracle's reset samplers against tests/golden/forced_rng_resets.npz (recorded from the
imported reference by tests/golden/make_golden_forced_rng.py), bit for bit.  The GPU part (test_forced_rng_gpu.py) runs the device
kernels against the oracle from the same states and imports the fixture / oracle plumbing from here."""
from __future__ import annotations

import copy
import ctypes as C
import json
from functools import lru_cache

import numpy as np
import pytest

import rng_forcing as rf
from conftest import GOLDEN
from oracle import oracle as orc
from oracle import route_oracle as ro
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg

# every class the fixture must hold, each at least twice (test_fixture_census)
CLASSES = ("u_zero", "u_max", "u_boundary", "u_boundary_minus", "u_boundary_plus", "rot0", "rot63", "lemire_zero", "lemire_reject",
           "lemire_at_threshold", "wedge_accept", "wedge_reject", "tail", "tail_retry", "pair_l2_exhausted", "pair_l2_later",
           "close_bucket_exhausted", "close_bucket_later", "zero_ratios")
FLOAT_KEYS = ("initial_q", "initial_dq", "initial_prev_action", "goal_q")


# ============================================================================== fixture and oracle plumbing (shared with the GPU tests)
@lru_cache(maxsize=None)
def fixture() -> dict:
    g = np.load(GOLDEN / "forced_rng_resets.npz")
    out = {k: g[k] for k in g.files if k != "groups"}
    out["groups"] = json.loads(str(g["groups"]))
    return out


def rows_of(group: str) -> np.ndarray:
    return np.flatnonzero(fixture()["group"] == group)


def group_cfg_dict(group: str, extra: dict | None = None) -> dict:
    """the resolved golden config of the group with its overrides ("a.b.c": value) applied, then `extra`"""
    g = fixture()["groups"][group]
    cfg = copy.deepcopy(json.loads((GOLDEN / "configs" / f"{g['config']}.json").read_text()))
    for path, value in {**g["overrides"], **(extra or {})}.items():
        node = cfg
        keys = path.split(".")
        for k in keys[:-1]:
            node = node.setdefault(k, {})
        node[keys[-1]] = value
    return cfg


def set_oracle_rng(r: orc.ORng, w) -> None:
    st = kcfg.RngState()
    (st.state_hi, st.state_lo, st.inc_hi, st.inc_lo, st.has_uint32, st.uinteger) = (int(x) for x in w)
    orc.lib().kp1o_rng_set(C.byref(r), C.byref(st))


def oracle_rng(w) -> orc.ORng:
    r = orc.ORng()
    set_oracle_rng(r, w)
    return r


@lru_cache(maxsize=None)
def _route() -> ro.Route:
    return ro.Route(rcfg.load_route_q(GOLDEN / "synthetic_route.json"))


class GroupOracle:
    """the oracle's sampler of one fixture group: sample(words) -> the row the fixture records (words after, floats, ints)"""

    def __init__(self, group: str) -> None:
        self.g = fixture()["groups"][group]
        cfgd = group_cfg_dict(group)
        self.base = kcfg.to_env_config(cfgd, handoff_base_dirs=(GOLDEN,))
        if self.g["kind"] == "route":
            self.rc = rcfg.route_config_from_dict(cfgd)
        else:
            self.env = orc.OracleEnv(self.base)
            self.env.set_curriculum_stage(self.g["stage"])
            assert len(self.base.handoff_states) == self.g["n_handoff"] or self.g["kind"] != "dock"

    def sample(self, w) -> dict:
        ints = [-1, -1, -1, -1]
        if self.g["kind"] == "route":
            L = ro.lib()
            r, s = oracle_rng(w), ro.RouteSample()
            L.kp1o_route_sample_reset(C.byref(r), _route()._h, C.byref(self.base.c.joints), C.byref(self.rc.reset), C.byref(s))
            out = {k: np.array(getattr(s, k)[:]) for k in FLOAT_KEYS}
            ints[:3] = [s.route_index, s.start_index, s.mode]
            after = orc.rng_words(r)
        else:
            set_oracle_rng(self.env.e.rng, w)
            self.env.reset()
            st = self.env.state()
            out = {"initial_q": st["q"], "initial_dq": st["dq"], "initial_prev_action": st["prev_action"], "goal_q": st["goal_q"]}
            ints[3] = int(self.env.e.last_reset_stage)
            after = self.env.rng_words()
        out.update(ints=np.array(ints, dtype=np.int64), words_after=after)
        return out


def classes_in(words: np.ndarray, draws: list, expect: list) -> list[str]:
    """the labels classify gives at the positions a fixture row names (CPU only: numpy replays the draws)"""
    got = rf.classify(words, draws)
    for at, want in expect:
        assert got[at][0] == want, (at, want, got[at])
    return [got[at][0] for at, _ in expect]


# ============================================================================== 1. the helper against numpy
@pytest.mark.parametrize("rot", [0, 1, 31, 32, 62, 63])
def test_forced_word_comes_out_of_random_raw(rot):
    rng = np.random.default_rng(rot)
    for inc in (rf.DEFAULT_INC, int(np.random.PCG64(99).state["state"]["inc"]), 1, rf.M128):
        for word in (0, rf.M64, 1, 1 << 63, int(rng.integers(0, 1 << 63)) * 2 + 1):
            hi = (rot << 58) | int(rng.integers(0, 1 << 58))
            w = rf.forced_words(word, hi=hi, inc=inc)
            bg = rf.bitgen_of(w)
            assert int(bg.random_raw()) == word
            assert int(rf.words_of(bg)[0]) == hi                    # the step landed on the chosen high half: rotation = rot
            assert rf.lcg_steps(w, rf.words_of(bg)) == 1


def test_buffered_half_and_lemire_values():
    for n in (170, 120, 40, 9, 6, 11, 94):
        t = rf.lemire_threshold(n)
        v, at = rf.lemire_rejected(n), rf.lemire_at_threshold(n)
        assert v > 0 and ((v * n) & 0xFFFFFFFF) < t and ((at * n) & 0xFFFFFFFF) == t
        for uint, label, steps in ((0, "lemire_reject", 1), (v, "lemire_reject", 1), (at, "integers", 0)):
            w = rf.forced_words(12345, hi=7 << 58, has_uint32=1, uinteger=uint)
            assert rf.classify(w, [("integers", 3, 3 + n)]) == [(label, steps)]
            if steps:   # numpy drew one fresh word and kept its high half
                g = rf.generator_of(w)
                g.integers(3, 3 + n)
                assert int(rf.words_of(g.bit_generator)[4]) == 1
    assert rf.lemire_rejected(170) == 25264514 and rf.lemire_threshold(170) == 86


def test_classify_labels_hand_built_cases():
    top = 0x000FFFFFFFFFFFFF           # the largest 52-bit magnitude: outside every layer's rectangle
    fast = rf.forced_words(0x37, hi=3 << 58)                                 # magnitude 0: inside the rectangle of layer 0x37
    assert rf.classify(fast, ["normal"]) == [("fast", 1)]
    tail = rf.forced_words((top ^ (1 << 8)) << 9, hi=9 << 58)                 # layer 0; bit 8 of the magnitude clear: positive tail
    (label, n), = rf.classify(tail, ["normal"])
    assert label in ("tail", "tail_retry") and n >= 3 and (n == 3) == (label == "tail")
    z = rf.generator_of(tail).standard_normal()
    assert z > rf.R
    tail_neg = rf.forced_words(top << 9, hi=9 << 58)                          # bit 8 of the magnitude set: negative tail
    assert rf.generator_of(tail_neg).standard_normal() < -rf.R
    wedge = rf.forced_words((top << 9) | 0x80, hi=40 << 58)                   # layer 128, far corner of the wedge: rejected
    (label, n), = rf.classify(wedge, ["normal"])
    assert label in ("wedge_reject", "tail", "tail_retry") and n >= 3
    assert rf.classify(rf.forced_words(rf.double_word(5), hi=1 << 58), ["double", "normal"])[0] == ("double", 1)
    # seeds found by the search reach the class at the position asked for
    draws = ["double", ("integers", 1, 171)] + ["normal"] * 21
    seed = rf.find_seed(draws, "wedge_accept", 5)
    assert rf.classify(rf.seed_words(seed), draws)[5] == ("wedge_accept", 2)
    seed = rf.find_seed(draws, "tail", 22, limit=20000)
    assert rf.classify(rf.seed_words(seed), draws)[22][0] == "tail"


# ============================================================================== 2. the oracle's primitives at forced states
def _states() -> list[np.ndarray]:
    rng = np.random.default_rng(5)
    out = []
    for rot in (0, 63, 1, 62, 17):
        for has, uint in ((0, 0), (1, 0), (1, 25264514), (1, 0xFFFFFFFF)):
            hi = (rot << 58) | int(rng.integers(0, 1 << 58))
            out.append(rf.forced_words(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), hi=hi, has_uint32=has, uinteger=uint,
                                       inc=int(rng.integers(0, 1 << 62)) * 2 + 1))
    return out


def _same_after(r: orc.ORng, g: np.random.Generator, ctx) -> None:
    assert np.array_equal(orc.rng_words(r), rf.words_of(g.bit_generator)), ctx


def test_oracle_primitives_at_forced_states():
    L = ro.lib()
    for i, w in enumerate(_states()):
        r, g = oracle_rng(w), rf.generator_of(w)
        assert L.kp1o_rng_next64(C.byref(r)) == int(g.bit_generator.random_raw()), i
        _same_after(r, g, i)
        r, g = oracle_rng(w), rf.generator_of(w)
        for k in range(3):     # buffered half first, then low half, then high half
            assert L.kp1o_rng_next32(C.byref(r)) == int(g.integers(0, 1 << 32, dtype=np.uint32)), (i, k)
            _same_after(r, g, (i, k))
        r, g = oracle_rng(w), rf.generator_of(w)
        assert L.kp1o_rng_double(C.byref(r)) == g.random(), i
        _same_after(r, g, i)
        for n in (170, 120, 40, 9, 6, 11, 94, 2, 1, 64):
            r, g = oracle_rng(w), rf.generator_of(w)
            for k in range(3):
                assert L.kp1o_rng_integers(C.byref(r), 1, 1 + n) == int(g.integers(1, 1 + n)), (i, n, k)
                _same_after(r, g, (i, n, k))
        r, g = oracle_rng(w), rf.generator_of(w)
        for k in range(4):
            assert L.kp1o_rng_standard_normal(C.byref(r)) == g.standard_normal(), (i, k)
            _same_after(r, g, (i, k))


def test_oracle_double_uniform_edges():
    L = ro.lib()
    for k in (0, 1, rf.ONE_BELOW, rf.ONE_BELOW - 1, rf.k_of(0.5), rf.k_of(0.5) - 1):
        for low11 in (0, 2047):
            w = rf.forced_words(rf.double_word(k, low11), hi=(63 << 58) | k)
            r = oracle_rng(w)
            u = L.kp1o_rng_double(C.byref(r))
            assert u == k * 2.0 ** -53 == rf.generator_of(w).random() and 0.0 <= u < 1.0


@pytest.mark.parametrize("n", [170, 120, 94, 9])
def test_oracle_double_lemire_rejection(n):
    """buffered half rejected, low half of the forced next word rejected, its high half accepted: two consecutive rejections, which no
    whole reset can be made to reach (the second rejected value would have to come out of the stream)"""
    L = ro.lib()
    v1, v2, ok = rf.lemire_rejected(n), rf.lemire_rejected(n, skip=1), 0x9E3779B9
    assert ((ok * n) & 0xFFFFFFFF) >= rf.lemire_threshold(n) and v1 != v2
    for first in (0, v1):
        for second in (0, v2):
            w = rf.forced_words((ok << 32) | second, hi=(0 if first else 63) << 58 | 77, has_uint32=1, uinteger=first)
            assert rf.classify(w, [("integers", 1, 1 + n)]) == [("lemire_reject", 1)]
            r, g = oracle_rng(w), rf.generator_of(w)
            got = L.kp1o_rng_integers(C.byref(r), 1, 1 + n)
            assert got == int(g.integers(1, 1 + n)) == 1 + ((ok * n) >> 32)
            _same_after(r, g, (n, first, second))
            assert int(orc.rng_words(r)[4]) == 0          # both halves of the one fresh word are spent


def test_oracle_standard_normal_ziggurat_classes():
    """the states of the fixture's ziggurat rows, advanced to the normal in question: value and words after against numpy"""
    L = ro.lib()
    f = fixture()
    seen = set()
    for i in np.flatnonzero(np.isin(f["cls"], ("wedge_accept", "wedge_reject", "tail", "tail_retry"))):
        draws = json.loads(str(f["draws"][i]))
        (at, want), = json.loads(str(f["expect"][i]))
        r, g = oracle_rng(f["words_before"][i]), rf.generator_of(f["words_before"][i])
        for d in draws[:at]:
            if d == "double":
                L.kp1o_rng_double(C.byref(r)), g.random()
            elif d == "normal":
                L.kp1o_rng_standard_normal(C.byref(r)), g.standard_normal()
            else:
                L.kp1o_rng_integers(C.byref(r), d[1], d[2]), g.integers(d[1], d[2])
        _same_after(r, g, i)
        here = rf.words_of(g.bit_generator)
        assert rf.classify(here, ["normal"])[0][0] == want
        z = L.kp1o_rng_standard_normal(C.byref(r))
        assert z == g.standard_normal() and (abs(z) > rf.R) == want.startswith("tail"), (i, want, z)
        _same_after(r, g, i)
        seen.add(want)
    assert seen == {"wedge_accept", "wedge_reject", "tail", "tail_retry"}


def test_oracle_choice_p_boundaries():
    """Generator.choice(p=) is searchsorted(cdf, u, side="right"): u exactly on a cdf entry belongs to the NEXT mode"""
    L = ro.lib()
    p = np.array([0.25, 0.25, 0.25, 0.125, 0.125])
    cdf = np.cumsum(p)
    for b, mode_at in ((0.25, 1), (0.5, 2), (0.75, 3), (0.875, 4)):
        for dk, want in ((-1, mode_at - 1), (0, mode_at), (1, mode_at)):
            k = rf.k_of(b) + dk
            w = rf.forced_words(rf.double_word(k, 1023), hi=(11 << 58) | k)
            r, g = oracle_rng(w), rf.generator_of(w)
            got = L.kp1o_rng_choice_p(C.byref(r), p.ctypes.data_as(C.POINTER(C.c_double)), 5)
            assert got == int(g.choice(5, p=p)) == want == int(np.searchsorted(cdf, k * 2.0 ** -53, side="right")), (b, dk)
            _same_after(r, g, (b, dk))
    for k, want in ((0, 0), (rf.ONE_BELOW, 4)):
        r = oracle_rng(rf.forced_words(rf.double_word(k), hi=5 << 58))
        assert L.kp1o_rng_choice_p(C.byref(r), p.ctypes.data_as(C.POINTER(C.c_double)), 5) == want


# ============================================================================== 3. the oracle's samplers against the fixture
@pytest.mark.parametrize("group", sorted(fixture()["groups"]))
def test_oracle_samplers_match_forced_fixture(group):
    f = fixture()
    ora = GroupOracle(group)
    idx = rows_of(group)
    assert idx.size > 0
    for i in idx:
        ctx = (group, str(f["label"][i]))
        w = f["words_before"][i]
        if f["u_k"][i] >= 0:
            assert rf.generator_of(w).random() == int(f["u_k"][i]) * 2.0 ** -53, ctx
        classes_in(w, json.loads(str(f["draws"][i])), json.loads(str(f["expect"][i])))
        got = ora.sample(w)
        assert np.array_equal(got["words_after"], f["words_after"][i]), ctx
        assert rf.lcg_steps(w, got["words_after"]) == int(f["words_used"][i]), ctx
        mask = f["ints"][i] >= 0
        assert np.array_equal(got["ints"][mask], f["ints"][i][mask]), (ctx, got["ints"], f["ints"][i])
        for k in FLOAT_KEYS:
            assert np.array_equal(got[k], f[k][i]), (ctx, k)


def test_boundary_rows_change_the_outcome():
    """the forced boundaries are real ones: where the fixture shows the branch taken, the reference puts u ON the boundary on the far side
    of it (`cdf[i] <= u`, `draw < cr`, `double < probability`) and u one ulp below on the near side, so `<` for `<=` cannot pass"""
    f = fixture()

    def rows(group: str, cls: str, k: int) -> np.ndarray:
        idx = rows_of(group)
        sel = idx[(f["cls"][idx] == cls) & (f["u_k"][idx] == k)]
        assert sel.size == 2, (group, cls, k)
        return sel

    for mode, b in enumerate((0.25, 0.5, 0.75, 0.875)):       # Generator.choice: searchsorted side="right"
        k = rf.k_of(b)
        assert np.all(f["ints"][rows("route170", "u_boundary_minus", k - 1), 2] == mode)
        assert np.all(f["ints"][rows("route170", "u_boundary", k), 2] == mode + 1)
        assert np.all(f["ints"][rows("route170", "u_boundary_plus", k + 1), 2] == mode + 1)
    k = rf.k_of(0.5)                                             # draw < current_stage_ratio keeps the current stage 9
    assert np.all(f["ints"][rows("ws9", "u_boundary_minus", k - 1), 3] == 9) and np.all(f["ints"][rows("ws9", "u_boundary", k), 3] < 9)
    # random() < handoff_state_probability: a hand-off reset is two words (the uniform and the index), any other at least fifteen
    assert np.all(f["words_used"][rows("dock_handoff", "u_boundary_minus", k - 1)] == 2) and np.all(f["words_used"][rows("dock_handoff", "u_boundary", k)] >= 15)


def test_fixture_census(capsys):
    """what the forced set holds; a class with fewer than two rows fails, so coverage cannot vanish silently"""
    f = fixture()
    census = {c: int(np.sum(f["cls"] == c)) for c in CLASSES}
    per_group = {g: sorted({str(c) for c in f["cls"][rows_of(g)]}) for g in sorted(f["groups"])}
    with capsys.disabled():
        print(f"\nforced_rng_resets.npz: {len(f['cls'])} rows; per class {json.dumps(census)}")
        for g, cs in per_group.items():
            print(f"  {g} ({f['groups'][g]['kind']}, {rows_of(g).size} rows): {', '.join(cs)}")
    assert set(str(c) for c in f["cls"]) <= set(CLASSES)
    thin = {c: n for c, n in census.items() if n < 2}
    assert not thin, thin
    # each forced class comes with at least two different streams / high halves
    for c in CLASSES[:10]:
        rows = np.flatnonzero(f["cls"] == c)
        assert len({tuple(f["words_before"][i][2:4]) for i in rows}) >= 2 and len({int(f["words_before"][i][0]) for i in rows}) >= 2, c
    # the ziggurat classes at the first, a middle and the last of the 21 normals of a route reset
    for c in ("wedge_accept", "wedge_reject", "tail", "tail_retry"):
        at = sorted({json.loads(str(f["expect"][i]))[0][0] for i in np.flatnonzero(f["cls"] == c)})
        assert at == [2, 12, 22], (c, at)
    # Lemire rejection reaches the route window (170 and 120), the stage-index draws and the dock hand-off index
    lem = {(str(f["group"][i]), tuple(json.loads(str(f["draws"][i]))[1][1:])) for i in np.flatnonzero(f["cls"] == "lemire_reject")}
    assert {("route170", (1, 171)), ("route120", (1, 121)), ("ws9", (0, 9)), ("rs10", (0, 9))} <= lem
    assert any(g == "dock_handoff" for g, _ in lem)
