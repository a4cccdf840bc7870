"""Data-parallel route curriculum on ONE GPU: per-step episode records (kp1_route_episode_records), the chunked multi-rank prefix tracker
(kp1_route_curriculum_observe_chunk) against the reference callback's recorded traces and against the per-step tracker, and the route
trainer with two gloo ranks on cuda:0 (the collectives are backend-agnostic torch.distributed calls; multi-GPU runs use RCCL)."""
from __future__ import annotations

import json
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from conftest import GOLDEN
from rl_brain_trainer_amd import config as kcfg
from rl_brain_trainer_amd import route_config as rcfg
from rl_brain_trainer_amd.route_curriculum import RoutePrefixCurriculumDevice, _CurriculumState, build_prefix_stages
from rl_brain_trainer_amd.route_env import RouteVecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPEN = dict(promotion_success_rate=0.0, promotion_route_ready_hit_rate=0.0, promotion_orientation_hit_rate=0.0, promotion_max_regression_rate=1.0)


def _cfg() -> dict:
    return json.loads((GOLDEN / "configs" / "route_curriculum_prefix120_routeobs_sequence2.json").read_text())


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _blocks(records: torch.Tensor, t0: int, chunk: int, world: int) -> torch.Tensor:
    """[world, chunk, n_local] rank-major block of steps t0 .. t0 + chunk - 1 of per-step records [T, N] (rank r = envs r * n_local ..)"""
    n = records.shape[1]
    return records[t0:t0 + chunk].reshape(chunk, world, n // world).permute(1, 0, 2).contiguous()


def test_chunk_tracker_matches_reference_callback():
    """The reference callback's recorded (dones, infos) traces (tests/golden/route_eval.json), loaded into the env's flag planes step by step
    as in test_route_ppo_gpu, turned into episode records on the device, split into 1 / 2 / 3 rank blocks and replayed 1 / 4 / 16 steps at a
    time: stage and episode count at every chunk end, the summary (promotion events, their rates and timesteps) and the reset window."""
    gold = json.loads((GOLDEN / "route_eval.json").read_text())
    cfgd = _cfg()
    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    kw = dict(stages=build_prefix_stages([20, 40, 80]), promotion_success_rate=0.75, promotion_route_ready_hit_rate=0.75, promotion_orientation_hit_rate=0.85,
              promotion_max_regression_rate=0.30, window_episodes=16, min_episodes_per_stage=24)
    n_promotions = 0
    for trace in gold["callback"]:
        n, T = len(trace["steps"][0]["dones"]), len(trace["steps"])
        env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), route_q, n, seed=2)
        recorder = RoutePrefixCurriculumDevice(**kw)
        recorder.attach(env)
        env.reset()
        info = env.info()
        views = [info["route_ready"], info["route_orientation_hit"], info["route_regression"]]
        records = torch.zeros((T, n), dtype=torch.uint8, device=DEV)
        for t, step in enumerate(trace["steps"]):
            infos = step["infos"]
            done = torch.tensor([(1 if d else 0) | (4 if (d and i["success"]) else 0) for d, i in zip(step["dones"], infos)], dtype=torch.uint8, device=DEV)
            # a success flag on a not-done env must be ignored, like info["success"] of an unfinished episode
            done |= torch.tensor([4 if (i["success"] and not d) else 0 for d, i in zip(step["dones"], infos)], dtype=torch.uint8, device=DEV)
            for v, key in zip(views, ("route_ready", "route_orientation_hit", "route_regression")):
                v.copy_(torch.tensor([int(i[key]) for i in infos], dtype=torch.uint8, device=DEV))
            recorder.record(done, records[t])
        recorder.close()
        for world in (1, 2, 3):
            for chunk in (1, 4, 16):
                cb = RoutePrefixCurriculumDevice(**kw)
                cb.attach(env)
                for t0 in range(0, T, chunk):
                    cb.observe_chunk(_blocks(records, t0, chunk, world), n // world, chunk, world)
                    st = cb.read()
                    want = trace["steps"][t0 + chunk - 1]
                    assert (int(st.stage_index), int(st.stage_episode_count)) == (want["stage"], want["count"]), (world, chunk, t0)
                summary = json.loads(json.dumps(cb.summary()))
                assert summary == trace["summary"], (world, chunk)
                assert env.route_cfg.reset.max_route_index == trace["summary"]["prefix_end_index"]
                env.reset()                                          # the device config carries the promoted window
                assert int(env.info()["route_index"].max()) <= trace["summary"]["prefix_end_index"]
                cb.close()
        n_promotions += len(trace["summary"]["history"])
        env.close()
    assert n_promotions == 2


def test_live_records_and_chunk_replay_equal_the_per_step_tracker():
    """512 servo-driven route envs with auto-reset and open promotion thresholds, the per-step tracker attached: after every step the
    records equal done | ready << 4 | orientation hit << 5 | regression << 6 of the env's flags, and the saved records replayed through the
    chunk tracker (virtual splits into 1 / 2 / 4 ranks, chunks of 1 / 8 / 16 steps) leave a tracker byte-identical to the live one."""
    cfgd = _cfg()
    cfgd["env"]["termination"]["max_episode_steps"] = 20          # truncations as well as successes end episodes within the 64 steps
    route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
    N, T = 512, 64
    kw = dict(stages=build_prefix_stages([5, 10, 20, 40, 80, 120]), window_episodes=48, min_episodes_per_stage=64, **OPEN)
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), route_q, N, seed=17)
    live = RoutePrefixCurriculumDevice(**kw)
    live.attach(env)
    obs = env.reset()
    records = torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    ended = 0
    for t in range(T):
        a = (0.8 * RouteVecEnv.obs_dict(obs)["route_q_error"]).clamp(-1, 1)
        obs, _, done = env.step(a)
        live.observe(done, N)
        live.record(done, records[t])
        flags = (env.episode_flags() != 0).to(torch.uint8)
        want = (done & 0x0F) | (flags[0] << 4) | (flags[1] << 5) | (flags[2] << 6)
        assert torch.equal(records[t], want), t
        ended += int((done & 3).ne(0).sum())
    ref = bytes(live.read())
    n_events = int(live.read().n_events)
    assert ended > 0 and n_events >= 2, (ended, n_events)      # the replay below crosses promotions
    live.close()
    env.close()

    env2 = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), route_q, 8, seed=1)
    for world in (1, 2, 4):
        for chunk in (1, 8, 16):
            cb = RoutePrefixCurriculumDevice(**kw)
            cb.attach(env2)
            for t0 in range(0, T, chunk):
                cb.observe_chunk(_blocks(records, t0, chunk, world), N // world, chunk, world)
            st = cb.read()
            assert bytes(st) == ref, (world, chunk)
            assert env2.route_cfg.reset.max_route_index == int(st.prefix_end_index[st.stage_index])
            cb.close()
    env2.close()


# ------------------------------------------------------------------------------------------------------------- through PPO / the trainer
def _dp_graph_worker(rank: int, world: int, port: int, out_dir: str) -> None:
    """the same route training run with graph segments and eagerly, data parallel: bit-identical results on every rank"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rl_brain_trainer_amd import ppo as P

        cfgd = _cfg()
        cfgd["env"]["termination"]["max_episode_steps"] = 12
        route_q = rcfg.load_route_q(GOLDEN / "synthetic_route.json")
        N = 128

        def run(use_graphs: bool):
            env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=120), route_q, N, seed=9, first_env_id=rank * N)
            cur = RoutePrefixCurriculumDevice(stages=build_prefix_stages([5, 10, 20, 40]), window_episodes=32, min_episodes_per_stage=32, **OPEN)
            pcfg = P.PPOConfig(n_steps=32, batch_size=1024 * world, n_epochs=2, hidden=256, learning_rate=3e-4, seed=5, clip_range=0.2, ent_coef=1e-3)
            ppo = P.PPO(env, pcfg, curriculum=cur, dist=P.Dist(), backend="hip", use_graphs=use_graphs)
            assert ppo.dist.enabled and ppo._record_stage is not None and ppo._record_stage.shape == (ppo.done_chunk, N)
            for it in range(3):
                # the route env has no device snapshot: iteration 0 runs eagerly in both forms (a step callback forces it), so the capture of
                # iteration 1 finds the kernels warm and does not restart the episodes; iterations 1 and 2 replay the graph segments
                ppo.step_callback = (lambda d: None) if it == 0 else None
                ppo.collect_rollouts()
                ppo.train()
            assert (ppo._rollout_graph is not None) == use_graphs
            torch.cuda.synchronize()
            out = (ppo.policy.flat.clone(), ppo.adam_m.clone(), ppo.adam_v.clone(), ppo.obs_buf.clone(), bytes(cur.read()))
            cur.close()
            env.close()
            return out

        seg, eager = run(True), run(False)
        for a, b in zip(seg[:4], eager[:4]):
            assert torch.equal(a, b)
        assert seg[4] == eager[4]
        both = [None] * world
        dist.all_gather_object(both, (seg[0].cpu().numpy(), seg[4]))
        assert np.array_equal(both[0][0], both[1][0]) and both[0][1] == both[1][1]
        assert _CurriculumState.from_buffer_copy(seg[4]).n_events >= 1
        Path(out_dir, f"ok{rank}").write_text("ok")
    finally:
        dist.destroy_process_group()


def test_route_dp_segmented_and_eager_rollouts_are_bit_identical(tmp_path):
    mp.spawn(_dp_graph_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()


def _train_worker(rank: int, world: int, port: int, out_dir: str, cfg_path: str, chunk: int) -> None:
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world),
                       "KP1_DONE_EXCHANGE_STEPS": str(chunk)})
    os.environ.pop("LOCAL_RANK", None)                                   # both ranks on cuda:0
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rl_brain_trainer_amd import train_route

        seen: dict = {}

        class RecordingPPO(train_route.PPO):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                seen["ppo"] = self

        class RecordingCurriculum(train_route.RoutePrefixCurriculumDevice):
            def close(self):
                if self.env is not None and self._st.value:
                    seen["tracker"] = bytes(self.read())
                super().close()

        train_route.PPO = RecordingPPO
        train_route.RoutePrefixCurriculumDevice = RecordingCurriculum
        out = Path(out_dir) / f"rank{rank}"
        summary = train_route.main(["--config", cfg_path, "--run-id", "dp", "--output-dir", str(out), "--total-timesteps", "16384", "--n-envs", "128",
                                    "--n-steps", "16", "--batch-size", "1024", "--seed", "4"])
        ppo = seen["ppo"]
        assert ppo.dist.world_size == world and ppo.done_chunk == chunk
        np.savez(Path(out_dir) / f"state{rank}.npz", flat=ppo.policy.flat.cpu().numpy(), m=ppo.adam_m.cpu().numpy(), v=ppo.adam_v.cpu().numpy(),
                 tracker=np.frombuffer(seen["tracker"], dtype=np.uint8), extra=np.array([ppo.actor_extra_steps, ppo.num_timesteps]))
        if rank == 0:
            (Path(out_dir) / "summary.json").write_text(json.dumps(summary, default=str))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("chunk", [16, 1])
def test_train_route_two_ranks(tmp_path, chunk):
    """train_route.main on two gloo ranks (128 envs each, open thresholds, teacher anchor and gate on): the ranks end in step (parameters,
    Adam moments, tracker bytes), one promotion on the global clock, rank 0 writes every artefact and rank 1 none."""
    cfgd = _cfg()
    cfgd["env"]["termination"]["max_episode_steps"] = 16               # every env ends an episode by step 16: the promotion comes early
    route_path = GOLDEN / "synthetic_route.json"
    route_q = rcfg.load_route_q(route_path)
    env = RouteVecEnv(kcfg.to_env_config(cfgd), rcfg.route_config_from_dict(cfgd, max_route_index=20), route_q, 64, seed=3)
    rows, acts, ridx = [], [], []
    obs = env.reset()
    for _ in range(20):
        d = RouteVecEnv.obs_dict(obs)
        a = (0.8 * d["route_q_error"]).clamp(-1, 1)
        rows.append(obs.cpu().numpy().copy())
        acts.append(a.cpu().numpy().copy())
        ridx.append(env.info()["route_index"].cpu().numpy().copy())
        obs, _, _ = env.step(a)
    env.close()
    rows, acts, ridx = np.concatenate(rows), np.concatenate(acts), np.concatenate(ridx)
    npz = tmp_path / "teacher.npz"
    np.savez(npz, actions=acts.astype(np.float32), route_index=ridx.astype(np.int32),
             **{f"obs__{k}": rows[:, o:o + w] for k, (o, w) in rcfg.ROUTE_OBS_LAYOUT.items()})
    cfgd["route"]["curriculum"] = {**cfgd["route"].get("curriculum", {}), "prefix_stages": [10, 20], "promotion_window_episodes": 32, "min_episodes_per_stage": 32,
                                   **OPEN}
    cfgd["route"]["teacher_anchor"] = {"enabled": True, "dataset_path": str(npz), "loss_weight": 0.02, "batch_size": 128, "max_route_index": 20}
    cfgd["route"]["sequential_gate"] = {"enabled": True, "prefixes": [5, 10], "full_end_index": 12}
    cfgd["route"]["route_path"] = str(route_path)
    cfgd["route"].pop("init_checkpoint", None)
    cfgd.setdefault("training", {})["checkpoint_freq"] = 4096
    cfg_path = tmp_path / "route.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgd))
    mp.spawn(_train_worker, args=(2, _free_port(), str(tmp_path), str(cfg_path), chunk), nprocs=2, join=True)

    s0, s1 = np.load(tmp_path / "state0.npz"), np.load(tmp_path / "state1.npz")
    for key in ("flat", "m", "v", "tracker", "extra"):
        assert np.array_equal(s0[key], s1[key]), key
    assert int(s0["extra"][0]) > 0                                       # the teacher anchor stepped
    summary = json.loads((tmp_path / "summary.json").read_text())
    assert summary["world_size"] == 2 and summary["n_envs"] == 256 and summary["env_steps_per_s"] > 0
    history = summary["curriculum_summary"]["history"]
    assert len(history) == 1 and summary["curriculum_summary"]["prefix_end_index"] == 20
    assert history[0]["total_timesteps"] > 0 and history[0]["total_timesteps"] % (2 * 128) == 0
    assert summary["teacher_anchor_summary"]["enabled"] and summary["route_gate_summary"]["schema_version"] == "v5.route_gate.v1"
    out0, out1 = tmp_path / "rank0", tmp_path / "rank1"
    for name in ("model_latest.zip", "curriculum_history.json", "training_summary.json", "route_eval_sequential/route_eval_sequential_summary.json",
                 "route_gate/route_gate_summary.json", "route_gate/full_12/route_eval_sequential_summary.json", "checkpoints/model_4096_steps.zip"):
        assert (out0 / name).exists(), name
    assert not out1.exists() or not any(out1.rglob("*"))
