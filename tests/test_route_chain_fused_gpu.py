"""The one-launch route chain evaluator (kp1_mlp_forward_route_chain_step, kp1_route_chain_run; RouteChain.forward_step / run;
evaluate_sequential_route_batch(form=)) against the same lock steps made by kp1_mlp_forward + kp1_route_chain_step on a twin handle.

Everything is compared bit for bit (torch.equal / np.array_equal): tags, the alive counter, the record table and its counts after every
call; for every row alive at a step its next_obs row, done, reward, action row, the env.info() planes and the wrapper's planes the chain
reads.  The launch-sequence chain goes on stepping a finished row and the one-launch forms do not: a finished row is compared at the step it
finished and is then asserted untouched.

Fixture: tests/test_route_chain_gpu.py's (imported, not edited) -- config route_curriculum_prefix120_routeobs_sequence2 with 24-step
episodes and `sequence` off, synthetic_route.json, END = 12, the servo nets at gain 0.6 (every waypoint reached) and 0.4 (waypoints 1-9
reached, 10-12 time out) and the seeded random net (none reached).  The servo nets read route_q_error, which the 56-float observation does not
carry: the 56-float cases run seeded random nets (hand-overs after truncations, no success) and the 80-float cases must show every outcome."""
from __future__ import annotations

import ctypes as C
import functools
import json
import warnings

import numpy as np
import pytest
import torch
import yaml

import test_route_chain_gpu as base
from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import native
from rl_brain_trainer_amd import route_config as rcfg

pytestmark = pytest.mark.gpu
DEV = base.DEV
END = base.END
STEPS = 24
PLANES = base.INFO_KEYS + ("nearest_route_q_distance", "route_waypoint_success", "route_regression", "route_orientation_hit",
                           "route_completed_waypoints", "start_route_index", "last_route_index")


def cfg_for(obs_dim: int) -> dict:
    cfgd = base.chain_cfg()
    cfgd["route"]["sequence"]["enabled"] = False
    cfgd["route"]["observation"] = {**cfgd["route"].get("observation", {}), "include_route_keys": obs_dim == 80}
    return cfgd


def make_env(n_rows: int, obs_dim: int, pitch: int, *, route_q=None, real: str = "f32", cfgd: dict | None = None):
    from rl_brain_trainer_amd.route_env import RouteVecEnv

    cfgd = cfgd or cfg_for(obs_dim)
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=END), base.route_q() if route_q is None else route_q,
                      n_rows, device=DEV, seed=0, real=real)
    assert env.obs_dim == obs_dim
    env.use_current_stream()
    env.set_obs_stride(pitch)
    return env


@functools.lru_cache(maxsize=None)
def nets(hidden: int, obs_dim: int):
    if obs_dim == 80:
        return base.policies(hidden)
    from rl_brain_trainer_amd.ppo import ActorCritic

    out = []
    for seed in (5, 6, 7):
        ac = ActorCritic(hidden, DEV, seed=seed, obs_dim=56)
        ac.views["action_net.weight"].mul_(base.RANDOM_HEAD_SCALE)
        out.append(ac)
    return tuple(out)


def make_mlp(hidden: int, obs_dim: int, members: tuple[int, ...], max_batch: int = 64):
    from rl_brain_trainer_amd import mlp

    h = mlp.MlpKernels(hidden, DEV, max_batch=max_batch, obs_dim=obs_dim, replicas=len(members))
    h.pack(torch.stack([nets(hidden, obs_dim)[p].flat for p in members]).contiguous())
    return h


def row_ends(K: int, C_: int) -> np.ndarray:
    return np.array([(12, 7, 1)[c % 3] for _ in range(K) for c in range(C_)], dtype=np.int32)


class Side:
    """one handle, one chain, its buffers; `fused` decides how a lock step is issued"""

    def __init__(self, mlp_handle, R: int, obs_dim: int, pitch: int, ends, stop: bool, *, in_place: bool = True, action: bool = True,
                 tags: bool = True) -> None:
        self.mlp, self.R = mlp_handle, R
        self.env = make_env(R, obs_dim, pitch)
        self.chain = self.env.chain(1, ends, stop_on_failure=stop)
        self.obs = torch.zeros((R, pitch), device=DEV)
        self.other = self.obs if in_place else torch.zeros((R, pitch), device=DEV)
        self.act = torch.full((R, 7), 9.0, device=DEV) if action else None
        self.reward = torch.full((R,), 9.0, device=DEV)
        self.done = torch.full((R,), 64, dtype=torch.uint8, device=DEV)
        self.tags = torch.full((R, 2), -7, dtype=torch.int32, device=DEV) if tags else None
        self.chain.begin(self.obs)
        info = self.env.info()
        self.planes = [info[k] for k in PLANES]

    def step_sequence(self) -> None:
        self.mlp.forward(self.obs, clipped=self.act)
        self.chain.step(self.act, self.other, self.reward, self.done, self.tags)
        self.obs, self.other = self.other, self.obs

    def step_fused(self) -> None:
        self.chain.forward_step(self.mlp, self.obs, self.other, self.reward, self.done, action=self.act, tags=self.tags)
        self.obs, self.other = self.other, self.obs

    def signature(self, with_action: bool = True) -> torch.Tensor:
        """[P, R] float64: every compared per-row value of this side (float32 and integers widen exactly)"""
        parts = [self.obs.t().double(), self.done.double()[None], self.reward.double()[None]]
        if self.act is not None and with_action:
            parts.append(self.act.t().double())
        parts += [p.reshape(-1, self.R).double() for p in self.planes]
        return torch.cat(parts)

    def table(self):
        return self.chain._records, self.chain._n_records

    def close(self) -> None:
        self.chain.close()
        self.env.close()


def plane_names(side: Side) -> list[str]:
    names = [f"obs[{c}]" for c in range(side.obs.shape[1])] + ["done", "reward"] + ([f"action[{c}]" for c in range(7)] if side.act is not None else [])
    for k, p in zip(PLANES, side.planes):
        names += [f"{k}[{j}]" for j in range(p.reshape(-1, side.R).shape[0])]
    return names


def assert_rows_equal(a: torch.Tensor, b: torch.Tensor, rows: torch.Tensor, side: Side, what) -> None:
    if torch.equal(a[:, rows], b[:, rows]):
        return
    bad = (a[:, rows] != b[:, rows]).nonzero()[0].tolist()
    r = int(rows.nonzero().flatten()[bad[1]])
    raise AssertionError((what, plane_names(side)[bad[0]], "row", r, float(a[bad[0], r]), float(b[bad[0], r])))


def events_of(tags: np.ndarray, dones: np.ndarray, K: int, C_: int) -> set[str]:
    """what the launch-sequence twin saw: tags [T, R, 2] and done bytes [T, R] after each lock step"""
    T, R = dones.shape
    alive = tags[:, :, 0] >= 0
    seen = set()
    if (alive[1:] & alive[:-1] & (tags[1:, :, 0] > tags[:-1, :, 0])).any():
        seen.add("hand-over")
    if (alive & ((dones & native.DONE_SUCCESS) != 0)).any():
        seen.add("success")
    if (alive & ((dones & native.DONE_TRUNCATED) != 0)).any():
        seen.add("truncation")
    last = alive.sum(axis=0)                      # a row is alive for a prefix of the steps: its count is the step it ended at
    if len(set(last.tolist())) > 1:
        seen.add("different-end-steps")
    tile = np.array([(r // C_) * 1000 + (r % C_) // 32 for r in range(R)])
    for t in range(T):
        tiles_alive = {int(x) for x in tile[alive[t]]}
        for g in set(tile.tolist()):
            rows = alive[t][tile == g]
            if rows.any() and not rows.all():
                seen.add("row-ends-inside-a-running-tile")
            if not rows.any() and tiles_alive:
                seen.add("tile-finished-while-another-runs")
    return seen


ALL_EVENTS = {"hand-over", "success", "truncation", "different-end-steps", "row-ends-inside-a-running-tile", "tile-finished-while-another-runs"}
STRUCTURAL = {"hand-over", "different-end-steps", "row-ends-inside-a-running-tile"}      # what per-row end indices give under any policy
#        hidden obs pitch members    C   in_place action tags  stop   events the reference run must show
CASES = [(64, 80, 128, (0, 1, 2), 33, True, True, True, False, ALL_EVENTS),
         (128, 80, 80, (0, 1, 2), 33, False, True, True, True, ALL_EVENTS),
         (128, 80, 128, (1,), 33, True, False, False, False, ALL_EVENTS),
         (64, 56, 64, (0, 1, 2), 33, False, False, True, False, STRUCTURAL | {"tile-finished-while-another-runs"}),
         (128, 56, 56, (1,), 33, True, True, False, False, STRUCTURAL | {"tile-finished-while-another-runs"}),
         (64, 80, 80, (1,), 1, True, True, True, True, {"hand-over", "success", "truncation"}),
         (64, 80, 128, (0, 1, 2), 2, False, True, True, False, ALL_EVENTS),
         (128, 56, 64, (2,), 2, True, True, True, False, STRUCTURAL)]


@pytest.mark.parametrize("hidden,obs_dim,pitch,members,C_,in_place,action,tags,stop,expect", CASES,
                         ids=[f"h{c[0]}-o{c[1]}p{c[2]}-K{len(c[3])}-C{c[4]}-{'inplace' if c[5] else 'separate'}{'-stop' if c[8] else ''}" for c in CASES])
def test_step_parity(hidden, obs_dim, pitch, members, C_, in_place, action, tags, stop, expect):
    """RouteChain.forward_step against forward + RouteChain.step on a twin handle, after every lock step up to the bound"""
    K = len(members)
    R = K * C_
    ends = row_ends(K, C_)
    mlp_handle = make_mlp(hidden, obs_dim, members)
    ref = Side(mlp_handle, R, obs_dim, pitch, ends, stop, in_place=in_place, action=True, tags=True)
    got = Side(mlp_handle, R, obs_dim, pitch, ends, stop, in_place=in_place, action=action, tags=tags)
    rng0, base_rng0 = got.env.rng_state().copy(), got.env.base.rng_state().copy()
    assert torch.equal(ref.obs, got.obs)
    bound = int(ends.max()) * STEPS
    prev = got.signature()
    all_tags, all_dones = [], []
    for step in range(bound):
        ref.step_sequence()
        got.step_fused()
        all_tags.append(ref.tags.clone())
        all_dones.append(ref.done.clone())
        alive = ref.tags[:, 0] >= 0            # the rows that were running when this step was taken
        if tags:
            assert torch.equal(got.tags, ref.tags), step
        assert got.chain._n_alive.item() == ref.chain._n_alive.item(), step
        for a, b in zip(got.table(), ref.table()):
            assert torch.equal(a, b), ("records", step)
        cur = got.signature()
        assert_rows_equal(cur, ref.signature(with_action=action), alive, got, ("alive rows", step))
        # (with two buffers a finished row's `obs` alternates between them: everything but the observation rows is checked)
        skip = 0 if in_place else pitch
        assert_rows_equal(cur[skip:], prev[skip:], ~alive, got, ("finished rows are untouched", step))
        prev = cur
    assert ref.chain.alive() == 0 and got.chain.alive() == 0
    seen = events_of(torch.stack(all_tags).cpu().numpy(), torch.stack(all_dones).cpu().numpy(), K, C_)
    print("reference events:", sorted(seen))
    assert set(expect) <= seen, (sorted(set(expect) - seen), "the launch-sequence twin did not show what this case is for")
    for a, b in zip(got.chain.records(), ref.chain.records()):
        assert np.array_equal(a, b)
    # neither form draws: both PCG64 streams of every row stand where they started
    assert np.array_equal(got.env.rng_state(), rng0) and np.array_equal(got.env.base.rng_state(), base_rng0)
    assert np.array_equal(ref.env.rng_state(), rng0) and np.array_equal(ref.env.base.rng_state(), base_rng0)
    ref.close()
    got.close()
    mlp_handle.close()


# ------------------------------------------------------------------------------------------------------------------- whole-chain parity
class Reference:
    """the per-step chain run to the bound once: after every lock step the alive counter, and each row's signature at its own last step"""

    def __init__(self, hidden: int, obs_dim: int, pitch: int, members, C_: int, stop: bool = False) -> None:
        K = len(members)
        self.R, self.ends = K * C_, row_ends(K, C_)
        self.mlp = make_mlp(hidden, obs_dim, members)
        side = Side(self.mlp, self.R, obs_dim, pitch, self.ends, stop, action=True, tags=True)
        self.bound = int(self.ends.max()) * STEPS
        last = side.signature(with_action=False)
        self.n_alive, self.last_at, self.n_records_at = [], [], []
        for _ in range(self.bound):
            side.step_sequence()
            alive = side.tags[:, 0] >= 0
            last = torch.where(alive[None], side.signature(with_action=False), last)
            self.n_alive.append(int(side.chain._n_alive.item()))
            self.last_at.append(last)
            self.n_records_at.append(side.chain._n_records.clone())
        self.records = side.chain.records()
        self.table = side.chain._records.clone()
        self.args = (obs_dim, pitch, stop)
        side.close()

    def fresh(self) -> Side:
        obs_dim, pitch, stop = self.args
        return Side(self.mlp, self.R, obs_dim, pitch, self.ends, stop, action=False, tags=False)


@functools.lru_cache(maxsize=None)
def whole_ref(hidden: int, obs_dim: int, pitch: int, members: tuple[int, ...], C_: int) -> Reference:
    ref = Reference(hidden, obs_dim, pitch, members, C_)
    assert ref.n_alive[-1] == 0
    assert len(set(ref.n_alive)) > 3, "rows must end at different lock steps"
    return ref


@pytest.mark.parametrize("hidden,obs_dim,pitch,members,split", [(64, 80, 128, (0, 1, 2), 0), (64, 80, 128, (0, 1, 2), 1), (64, 80, 128, (0, 1, 2), 7),
                                                                (64, 80, 128, (0, 1, 2), 32), (128, 80, 80, (0, 1, 2), 32), (64, 56, 64, (0, 1, 2), 7),
                                                                (128, 56, 56, (1,), 0)])
def test_whole_chain_parity(hidden, obs_dim, pitch, members, split):
    """kp1_route_chain_run for any split of the bound into consecutive calls (0: one call to the bound) against the per-step chain: after every
    call the alive counter, the record counts and every row's signature as of its own last step; then one more call with every row ended"""
    ref = whole_ref(hidden, obs_dim, pitch, members, 33)
    got = ref.fresh()
    steps = 0
    while steps < ref.bound:
        n = min(split or ref.bound, ref.bound - steps)
        got.chain.run(ref.mlp, got.obs, got.reward, got.done, n)
        steps += n
        assert got.chain.alive() == ref.n_alive[steps - 1], steps
        assert torch.equal(got.chain._n_records, ref.n_records_at[steps - 1]), steps
        assert_rows_equal(got.signature(), ref.last_at[steps - 1], torch.ones(ref.R, dtype=torch.bool, device=DEV), got, ("after lock step", steps))
    assert torch.equal(got.chain._records, ref.table)
    for a, b in zip(got.chain.records(), ref.records):
        assert np.array_equal(a, b)
    # every row has ended: another call writes nothing and leaves the counter at zero
    assert got.chain.alive() == 0
    before, table = got.signature(), got.chain._records.clone()
    got.chain.run(ref.mlp, got.obs, got.reward, got.done, 5)
    assert got.chain.alive() == 0 and torch.equal(got.signature(), before) and torch.equal(got.chain._records, table)
    got.close()


def test_whole_chain_span_cap_with_a_longer_bound():
    """a request above the cap (2200 lock steps) is run as calls of the cap: the first call's span is far longer than the chains, whose rows
    end inside it, and the later launches find no alive row and leave at once, so the test stays short"""
    ref = whole_ref(64, 80, 128, (0, 1, 2), 33)
    got = ref.fresh()
    cap = native.ROUTE_CHAIN_RUN_MAX_STEPS
    assert ref.bound < cap
    bound, steps = 2200, 0
    while steps < bound:
        n = min(cap, bound - steps)
        got.chain.run(ref.mlp, got.obs, got.reward, got.done, n)
        steps += n
        assert got.chain.alive() == 0
    assert steps == bound
    assert_rows_equal(got.signature(), ref.last_at[-1], torch.ones(ref.R, dtype=torch.bool, device=DEV), got, "after the cap-sized calls")
    assert torch.equal(got.chain._records, ref.table)
    got.close()


# ------------------------------------------------------------------------------------------------------------------------------- host
def _strip(result: dict) -> dict:
    return {k: v for k, v in result.items() if k != "lock_steps"}


def test_batch_evaluator_forms_agree(tmp_path, monkeypatch):
    from rl_brain_trainer_amd import route_curriculum as rc

    ends = (12, 7, 1)
    pop = base.population_mlp(64, (0, 1, 2))
    L = native.load()
    calls = {"kp1_route_chain_step": 0, "kp1_mlp_forward": 0, "kp1_mlp_forward_route_chain_step": 0, "kp1_route_chain_run": 0}

    def counted(name):
        fn = getattr(L, name)

        def call(*args):
            calls[name] += 1
            return fn(*args)
        return call

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    out = {}
    for form in rc.CHAIN_FORMS:
        for k in calls:
            calls[k] = 0
        out[form] = rc.evaluate_sequential_route_batch(mlp=pop, cfg=base.chain_cfg(), route_q=base.route_q(), start_index=1, end_indices=ends, device=DEV,
                                                       form=form, steps_per_launch=32, artifact_roots=[tmp_path / form / str(k) for k in range(3)])
        steps = out[form][0]["lock_steps"]
        if form == "launch_sequence":
            assert calls == {"kp1_route_chain_step": steps, "kp1_mlp_forward": steps, "kp1_mlp_forward_route_chain_step": 0, "kp1_route_chain_run": 0}
        elif form == "one_launch_step":
            assert calls == {"kp1_route_chain_step": 0, "kp1_mlp_forward": 0, "kp1_mlp_forward_route_chain_step": steps, "kp1_route_chain_run": 0}
        else:
            assert calls == {"kp1_route_chain_step": 0, "kp1_mlp_forward": 0, "kp1_mlp_forward_route_chain_step": 0, "kp1_route_chain_run": -(-steps // 32)}
    ref = out["launch_sequence"]
    for k, e in enumerate(ends):
        base.assert_same_result(ref[k], base.reference(64, k, 1, e), k)
    for form in ("one_launch_step", "whole_chain"):
        for k in range(3):
            assert out[form][k] == ref[k], (form, k)          # lock_steps included: equal at steps_per_launch = 32
            base.assert_same_files(tmp_path / form / str(k), tmp_path / "launch_sequence" / str(k), (form, k))
    # a larger span: the same results, lock_steps rounded up to the span (never past the bound)
    needed = max(sum(r["steps"] for r in ref[k]["rows"]) for k in range(3))
    wide = rc.evaluate_sequential_route_batch(mlp=pop, cfg=base.chain_cfg(), route_q=base.route_q(), start_index=1, end_indices=ends, device=DEV,
                                              form="whole_chain", steps_per_launch=100)
    assert [_strip(w) for w in wide] == [_strip(r) for r in ref]
    assert wide[0]["lock_steps"] == rc.chain_lock_steps(needed, 100, 12 * STEPS) and ref[0]["lock_steps"] == rc.chain_lock_steps(needed, 32, 12 * STEPS)
    pop.close()


def test_recorder_cli_one_launch_gives_the_same_arrays(tmp_path):
    from rl_brain_trainer_amd import collect_route_teacher

    p = base._failing_policy()
    ckpt = tmp_path / "teacher.pth"
    torch.save(base.policies(64)[p].state_dict(), ckpt)
    cfgd = base.chain_cfg()
    cfgd["route"].pop("init_checkpoint", None)
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    common = ["--checkpoint", str(ckpt), "--config", str(cfg_path), "--route-path", str(GOLDEN / "synthetic_route.json"), "--start-index", "1",
              "--end-index", str(END)]
    a = collect_route_teacher.main(common + ["--artifact-root", str(tmp_path / "seq")])
    b = collect_route_teacher.main(common + ["--artifact-root", str(tmp_path / "one"), "--one-launch"])
    assert {k: v for k, v in a.items() if k != "dataset_path"} == {k: v for k, v in b.items() if k != "dataset_path"}
    assert a["successful_indices"] and a["failed_indices"] and a["sample_count"] > 0
    with np.load(tmp_path / "seq" / "teacher_route_anchor_dataset.npz") as x, np.load(tmp_path / "one" / "teacher_route_anchor_dataset.npz") as y:
        assert sorted(x.files) == sorted(y.files)
        for key in x.files:
            assert x[key].dtype == y[key].dtype and np.array_equal(x[key], y[key]), key
    assert (tmp_path / "seq" / "teacher_route_anchor_dataset.npz").read_bytes() == (tmp_path / "one" / "teacher_route_anchor_dataset.npz").read_bytes()


def test_train_route_seeds_whole_chain_equals_the_default(tmp_path):
    from rl_brain_trainer_amd import train_route

    cfgd = base.chain_cfg()
    cfgd["route"]["curriculum"] = {**cfgd["route"].get("curriculum", {}), "prefix_stages": [4, 6], "promotion_window_episodes": 16,
                                   "min_episodes_per_stage": 16, "promotion_success_rate": 0.0, "promotion_route_ready_hit_rate": 0.0,
                                   "promotion_orientation_hit_rate": 0.0, "promotion_max_regression_rate": 1.0}
    cfgd["route"]["teacher_anchor"] = {"enabled": False}
    cfgd["route"]["sequential_gate"] = {"enabled": True, "prefixes": [3, 5], "full_end_index": 8}
    cfgd["route"]["route_path"] = str(GOLDEN / "synthetic_route.json")
    cfgd["route"].pop("init_checkpoint", None)
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    common = ["--config", str(cfg_path), "--n-envs", "16", "--n-steps", "64", "--batch-size", "256", "--hidden", "64", "--total-timesteps", "2048",
              "--seeds", "7,8", "--run-id", "t"]
    roots = {"whole": tmp_path / "whole", "default": tmp_path / "default"}
    train_route.main(common + ["--output-dir", str(roots["whole"]), "--chain-eval-form", "whole-chain"])
    train_route.main(common + ["--output-dir", str(roots["default"])])
    compared = 0
    for s in (7, 8):
        a, b = roots["whole"] / f"seed_{s}", roots["default"] / f"seed_{s}"
        files = sorted(p.relative_to(b) for d in ("route_eval_sequential", "route_gate") for p in (b / d).rglob("*") if p.is_file())
        assert len(files) == 4 + 3 * 4 + 1, files
        assert files == sorted(p.relative_to(a) for d in ("route_eval_sequential", "route_gate") for p in (a / d).rglob("*") if p.is_file())
        for f in files:
            assert base._normalised(a / f, roots["whole"]) == base._normalised(b / f, roots["default"]), (s, f)
            compared += 1
    assert compared == 34


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """every refusal of the two entry points: a status, kp1_last_error text, and nothing written"""
    from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, build_prefix_stages
    from rl_brain_trainer_amd.route_env import RoutePopulationVecEnv

    L = native.load()
    R, pitch = 6, 128
    mlp3 = make_mlp(64, 80, (0, 1, 2))
    env = make_env(R, 80, pitch)
    chain = env.chain(1, 3)
    obs = torch.zeros((R + 1, pitch), device=DEV)
    chain.begin(obs)
    bufs = {"obs": obs, "next": torch.full((R, pitch), 3.0, device=DEV), "act": torch.full((R, 7), 9.0, device=DEV),
            "reward": torch.full((R,), 9.0, device=DEV), "done": torch.full((R,), 64, dtype=torch.uint8, device=DEV),
            "tags": torch.full((R, 2), -7, dtype=torch.int32, device=DEV)}
    stream = mlp3._stream()

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def snapshot(e, c):
        return [t.clone() for t in bufs.values()] + [c._records.clone(), c._n_records.clone(), c._n_alive.clone()] + [e.info()[k].clone() for k in PLANES]

    def refused(text, *, m=mlp3, e=env, c=chain, o=obs, stride=pitch, nxt="next", n_steps=4, null=None, step=True, run=True):
        before = snapshot(e, c)
        args = {"m": m._h, "r": e._handle, "c": c._h, "obs": ptr(o), "act": ptr(bufs["act"]), "next": ptr(bufs[nxt]) if isinstance(nxt, str) else ptr(nxt),
                "reward": ptr(bufs["reward"]), "done": ptr(bufs["done"]), "tags": ptr(bufs["tags"])}
        if null:
            args[null] = None
        if step:
            rc = L.kp1_mlp_forward_route_chain_step(args["m"], args["r"], args["c"], args["obs"], stride, args["act"], args["next"], args["reward"],
                                                    args["done"], args["tags"], stream)
            assert rc != native.KP1_OK and text in L.kp1_last_error().decode(), (text, rc, L.kp1_last_error())
            with pytest.raises((ValueError, native.Kp1Error)):
                native.check(rc)
        if run and null not in ("next",):
            rc = L.kp1_route_chain_run(args["m"], args["r"], args["c"], args["obs"], stride, args["reward"], args["done"], n_steps, stream)
            assert rc != native.KP1_OK and text in L.kp1_last_error().decode(), (text, rc, L.kp1_last_error())
        torch.cuda.synchronize()
        for x, y in zip(snapshot(e, c), before):
            assert torch.equal(x, y), text

    for null in ("m", "r", "c", "obs", "next", "reward", "done"):
        refused("NULL argument", null=null)
    wide = base_mlp(256)
    refused("hidden 256", m=wide)
    wide.close()
    narrow = make_mlp(64, 56, (0, 1, 2))
    refused("obs_dim differs", m=narrow)
    narrow.close()
    refused("obs_stride must be", stride=96)
    refused("kp1_route_set_obs_stride", stride=80)
    four = make_mlp(64, 80, (0, 1, 2, 0))
    refused("multiple of the handle's replica count", m=four)      # 6 rows, 4 replicas
    four.close()
    refused("n_steps must be", n_steps=0, step=False)
    refused("n_steps must be", n_steps=native.ROUTE_CHAIN_RUN_MAX_STEPS + 1, step=False)
    refused("must be obs itself", nxt=obs[1:], run=False)           # shifted by one row: partial overlap
    # a chain of another handle
    other = make_env(R, 80, pitch)
    theirs = other.chain(1, 3)
    refused("belongs to another route handle", c=theirs)
    # what a chain cannot run on, switched on after the chain was made
    env.enable_reward_components(True)
    refused("reward components")
    env.enable_reward_components(False)
    cur = RoutePrefixCurriculumDevice(stages=build_prefix_stages([4, 6]), promotion_success_rate=0.8, promotion_route_ready_hit_rate=0.8,
                                      promotion_orientation_hit_rate=0.9, promotion_max_regression_rate=0.2, window_episodes=16)
    cur.attach(env)
    refused("tracker")
    cur.close()
    # handles no chain can be made on take another handle's chain: the handle's own refusal comes first
    seq = make_env(R, 80, pitch, cfgd={**base.chain_cfg()})
    refused("sequence", e=seq, c=theirs)
    seq.close()
    f64 = make_env(R, 80, pitch, real="f64")
    refused("f32", e=f64, c=theirs)
    f64.close()
    # a population route handle of 2 replicas under a policy handle of 3
    cfgd = cfg_for(80)
    pop_env = RoutePopulationVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=END), base.route_q(), [1, 2], 3, device=DEV)
    pop_env.set_obs_stride(pitch)
    pop_chain = pop_env.chain(1, 3)
    refused("replica count differs", e=pop_env, c=pop_chain)
    pop_chain.close()
    pop_env.close()
    # a route longer than the LDS overlay holds
    q = base.route_q()
    W = 920
    x = np.linspace(0, q.shape[0] - 1, W)
    long_q = np.stack([np.interp(x, np.arange(q.shape[0]), q[:, j]) for j in range(q.shape[1])], axis=1)
    long_env = make_env(R, 80, pitch, route_q=long_q)
    long_chain = long_env.chain(1, 3)
    refused("KP1_ROUTE_FUSED_MAX_WAYPOINTS", e=long_env, c=long_chain)
    long_chain.close()
    long_env.close()
    if torch.cuda.device_count() < 2:
        warnings.warn("one GPU: the different-devices refusal of the one-launch chain step is not exercised")
    # the one-launch rollout step keeps refusing a handle with a live chain
    noise = torch.zeros((R, 7), device=DEV)
    rc_ = L.kp1_mlp_forward_route_step(mlp3._h, env._handle, ptr(obs), pitch, ptr(noise), None, ptr(bufs["act"]), None, ptr(bufs["next"]), ptr(bufs["reward"]),
                                       ptr(bufs["done"]), None, stream)
    assert rc_ != native.KP1_OK and b"live kp1_route_chain" in L.kp1_last_error()
    # and the accepted call still works afterwards
    chain.forward_step(mlp3, obs[:R], obs[:R], bufs["reward"], bufs["done"])
    assert chain.alive() == R
    theirs.close()
    other.close()
    chain.close()
    env.close()
    mlp3.close()


def base_mlp(hidden: int):
    from rl_brain_trainer_amd import mlp

    return mlp.MlpKernels(hidden, DEV, max_batch=8, obs_dim=80, replicas=1)
