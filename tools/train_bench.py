"""Microseconds per train step (DQNTeamTrainer.train_step, src/train.py:50-149): the torch path vs the HIP path
(susnet_dqn_train_step), at several batch sizes, plus the trainer cadence at 65 536 envs (one 5-tick collect block + one train step
at batch 32).  Prints one JSON line."""
import argparse
import copy
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

pkg = importlib.import_module("sus-net_amd")
COMPS3 = ["onehot_pos", "alive_crew", "closest_crew"]


def game(name, batch):
    if name == "1v2":
        env = pkg.BatchedFourRoomEnv(1, 2, 4, batch=batch, device="cuda:0", rng="philox", seed=5, auto_reset=True, grid_size=14,
                                     shuffle_imposter_index=True, obs=pkg.ObsConfig("flat", COMPS3), check_errors=False)
        return env, COMPS3, True
    kw = dict(n_crew=1, n_jobs=0, kill_reward=-3, sabotage_reward=0, end_of_game_reward=0, time_step_reward=0)
    env = pkg.BatchedImposterTrainingGround(**kw, grid=pkg.four_room_grid(9, False), batch=batch, device="cuda:0", rng="philox", seed=6,
                                            auto_reset=True, obs=pkg.ObsConfig("flat", ["onehot_pos"]), check_errors=False)
    return env, ["onehot_pos"], False


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8,32,4096,65536")
    args = ap.parse_args()
    out = {"unit": "us_per_train_step", "games": {}}
    for name in ("1v2", "1v1"):
        env, comps, crew = game(name, 4096)
        ring = pkg.DeviceReplayBuffer(4096 * 16, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
        ring.populate_fused(env, 16)
        imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
        cr = pkg.policy.reference_crew_mlp(env, comps, seed=4) if crew else None
        hip = pkg.DeviceDQNTeamTrainer(env, imp, cr, comps, 1e-4, 0.9, train_crew=crew)
        ref = pkg.DeviceDQNTeamTrainer(env, copy.deepcopy(imp), copy.deepcopy(cr), comps, 1e-4, 0.9, train_crew=crew)
        ref.hip = False
        rows = {}
        for n in [int(x) for x in args.sizes.split(",")]:
            idx = torch.randint(0, ring.size, (n,), device="cuda:0")
            t_torch = timed(lambda: ref.train_step_on_indices(ring, idx), args.steps, args.warmup)
            t_hip = timed(lambda: hip.train_step_on_indices(ring, idx), args.steps, args.warmup)
            rows[str(n)] = {"torch": round(t_torch, 1), "hip": round(t_hip, 1), "speedup": round(t_torch / t_hip, 2)}
        out["games"][name] = rows
        del env, ring
    # trainer cadence at 65 536 envs on the 1v2 game: one 5-tick collect block + one train step at batch 32
    env, comps, _ = game("1v2", 65536)
    ring = pkg.DeviceReplayBuffer(65536 * 10, env.flattened_state_size, 1, env.n_agents, env.n_imposters, device=env.device)
    imp = pkg.policy.reference_imposter_mlp(env, comps, seed=3)
    cr = pkg.policy.reference_crew_mlp(env, comps, seed=4)
    cad = {}
    for path in ("torch", "hip"):
        m_imp, m_cr = copy.deepcopy(imp), copy.deepcopy(cr)
        pol = pkg.PolicyRollout(env, m_imp, None, comps)
        tr = pkg.DeviceDQNTeamTrainer(env, m_imp, m_cr, comps, 1e-4, 0.9, policy=pol)
        tr.hip = tr.hip and path == "hip"
        env.reset()
        ring.collect(env, pol, 5, ticks_per_append=5)

        def cycle():
            ring.collect(env, pol, 5, ticks_per_append=5)
            tr.train_step(ring, 32)
        cad[path] = round(timed(cycle, max(5, args.steps // 2), 2), 1)
    out["cadence_65536_envs_5_ticks_plus_step_b32"] = cad
    print(json.dumps(out))


if __name__ == "__main__":
    main()
