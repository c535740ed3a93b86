"""Dropout between the SpatialDQN's RNN layers in the train step, on the MI355X: the library's masks (susnet_rnn_dropout_mask) as
include/susnet.h states them, the dropout train step (susnet_spatial_train_step_dropout) against torch autograd through the float64
restatement, and run_experiment end to end on the reference's own kind of network (three RNN layers, rnn_dropout 0.2).  The restatement
(spatial_dropout_util.py) is pinned to the reference's module by test_spatial_dropout_host.py; the masks it is fed here are the
library's own.

Shapes: 33 rows (row tile 32): a ragged second tile; H = 12 and 33 (below one 32-unit block, and one unit into the second; 33 is no
multiple of the four units of a Philox block); T = 2 and 3; L = 2 and 3 (at L = 3 the middle layer has a mask on both sides); and once the
notebook's recurrence and head, H = 64, L = 3, T = 6, head [16, 16]."""
import copy
import ctypes as C
import importlib
import json
import math

import numpy as np
import pytest
import torch

from spatial_dropout_util import export_mask, make_drop, masked_train_step
from spatial_train_util import SpatialCall, agent_feats, as_global, compare_tensors, make_batch, make_model
from train_exact import DEV, _workspace

pytestmark = pytest.mark.gpu

N5, C3, A3 = 5, 3, 3
SEED = 1  # the one mask seed of this file (the kept-fraction condition below is a statement about THIS seed's masks)


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def env3(pkg):
    """A 3-agent, one-imposter handle: the network entry points take the agent and imposter counts from it and nothing else."""
    return pkg.BatchedFourRoomEnv(1, 2, 4, batch=64, device=DEV, rng="philox", seed=3, auto_reset=True, grid_size=9)


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(key, ctr):
    """Philox4x32-10 on one counter block (Salmon et al., SC'11), in Python integers."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def header_mask(p, seed, offset, net, agent, row, t, layer, unit):
    """include/susnet.h's statement of the multiplier, restated."""
    p32 = float(np.float32(p))
    g = row
    ctr = (unit // 4 | layer << 8 | t << 12 | net << 16 | agent << 20, g & 0xFFFFFFFF, (g >> 32) & 0xFF | (offset >> 32) << 8, offset & 0xFFFFFFFF)
    word = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), ctr)[unit % 4]
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if word >= math.floor(p32 * 2.0 ** 32) else 0.0


@pytest.mark.parametrize("p", [0.2, 0.5])
def test_mask_export(pkg, env3, p):
    L = pkg._lib
    layers, n, T, H = 3, 33, 3, 33
    base = dict(p_online=p, p_target=p, seed=SEED, offset=5, row_base=0)
    get = lambda net=0, agent=0, rows=n, **kw: export_mask(pkg, env3, make_drop(L, **dict(base, **kw)), net, agent, layers, rows, T, H)
    m = get()
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert m.dtype == np.float32 and np.isin(m, (np.float32(0.0), s)).all(), "multipliers are 0 or 1 / (1 - p) in float32, exactly"
    assert np.array_equal(m.view(np.int32), get().view(np.int32)), "equal arguments, equal bytes"
    # every input of the function matters
    for what, other in (("seed", get(seed=SEED + 1)), ("seed hi", get(seed=SEED + (1 << 32))), ("offset", get(offset=6)),
                        ("offset hi", get(offset=5 + (1 << 32))), ("net", get(net=1)), ("agent", get(agent=1)), ("row_base", get(row_base=1)),
                        ("row_base hi", get(row_base=1 << 32))):
        assert not np.array_equal(m, other), what
    assert not np.array_equal(m[0], m[1]), "layer"
    assert not np.array_equal(m[:, :, 0], m[:, :, 1]) and not np.array_equal(m[:, :, 1], m[:, :, 2]), "t"
    assert not np.array_equal(m[:, 0], m[:, 1]), "row"
    assert np.array_equal(get(row_base=1)[:, :-1], m[:, 1:]), "row_base is added to the row"
    # rows [k, k + 8) of a batch are those rows taken alone
    for k in (0, 7, 25):
        assert np.array_equal(get(rows=8, row_base=k), m[:, k:k + 8]), k
    # the header's statement of the function, element by element on a sample that covers every layer, step, word and the last (ragged) unit
    rng = np.random.default_rng(3)
    sample = [(int(rng.integers(layers - 1)), int(rng.integers(n)), int(rng.integers(T)), int(rng.integers(H))) for _ in range(200)]
    sample += [(l, r, t, u) for l in range(layers - 1) for r in (0, n - 1) for t in range(T) for u in (0, 1, 2, 3, H - 2, H - 1)]
    for l, r, t, u in sample:
        assert m[l, r, t, u] == header_mask(p, SEED, 5, 0, 0, r, t, l, u), (l, r, t, u)
    hi = get(net=1, agent=2, offset=(3 << 32) + 9, row_base=(1 << 33) + 4, rows=2)
    assert hi[1, 1, 2, 32] == header_mask(p, SEED, (3 << 32) + 9, 1, 2, (1 << 33) + 5, 2, 1, 32)
    # the kept fraction over N = 33 x 3 x 33 x 2 elements: a condition on a deterministic value -- seed 1, offset 5 -- not a retry loop
    N = m.size
    assert N == 33 * 3 * 33 * 2
    kept = float((m != 0).mean())
    print(f"p = {p}: kept {kept:.5f} of {N}, expected {1 - p} +- {5 * math.sqrt(p * (1 - p) / N):.5f}")
    assert abs(kept - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / N)
    # p = 0 keeps everything: 1.0f
    assert (get(p_online=0.0) == 1.0).all()


# ---- 7. the train step -----------------------------------------------------------------------------------------------------------------------
class DropoutCall(SpatialCall):
    """SpatialCall through susnet_spatial_train_step_dropout: ``drops`` = [imposter, crew] susnet_rnn_dropout, the workspace from the
    dropout form's own query."""

    def __init__(self, pkg, env, models, targets, batch, gamma, drops, **kw):
        super().__init__(pkg, env, models, targets, batch, gamma, **kw)
        L = pkg._lib
        self.drops = (L.RnnDropout * 2)(*drops)
        nbytes = C.c_uint64()
        L.check(env.lib.susnet_spatial_train_dropout_workspace_bytes(env._h, C.byref(self.io), C.byref(nbytes)))
        assert nbytes.value >= self.nbytes
        self.nbytes = int(nbytes.value)
        self.ws = _workspace(self.nbytes)
        self.io.workspace, self.io.workspace_bytes = self.ws.data_ptr(), self.nbytes

    def launch(self):
        self.pkg._lib.check(self.env.lib.susnet_spatial_train_step_dropout(self.env._h, C.byref(self.io), self.drops, self.env._stream()))


def _drops(pkg, p_online, p_target, offset=0, seed=SEED):
    return [make_drop(pkg._lib, p_online, p_target, seed=seed, offset=offset) for _ in range(2)]


def _library_masks(pkg, env, models, drops, n, T, A):
    """masks[(agent, team)] = (online, target), each [L - 1][n, T, H] float64: row = the position in the batch."""
    out = {}
    for agent in range(A):
        for team, m in enumerate(models):
            if m is None:
                continue
            rnn = m.rnn.model
            if rnn.num_layers < 2:
                out[agent, team] = (None, None)
                continue
            get = lambda net: list(torch.as_tensor(export_mask(pkg, env, drops[team], net, agent, rnn.num_layers, n, T, rnn.hidden_size)).double())
            out[agent, team] = (get(0), get(1))
    return out


def masked_reference(pkg, models, targets, batch, gamma, lr, masks):
    """One masked_train_step on float64 CPU copies: (losses [2], exp_avg per team as flat float64, Adam step counts)."""
    ms = [m and copy.deepcopy(m).cpu().double() for m in models]
    ts = [t and copy.deepcopy(t).cpu().double() for t in targets]
    opts = [m and torch.optim.Adam(m.parameters(), lr=lr) for m in ms]
    idx = torch.as_tensor(batch["idx"])
    sf, nf = agent_feats(batch, "spatial", torch.float64), agent_feats(batch, "next_spatial", torch.float64)
    losses = masked_train_step(ms, ts, opts, gamma, sf, nf, torch.as_tensor(batch["actions"])[idx].long(),
                               torch.as_tensor(batch["rewards"])[idx].double(), torch.as_tensor(batch["dones"])[idx].bool().reshape(-1, 1),
                               torch.as_tensor(batch["imposters"])[idx].to(torch.int16).reshape(-1, 1), masks)
    ea, counts = [], []
    for m, o in zip(ms, opts):
        if m is None:
            ea.append(None), counts.append(0.0)
            continue
        ea.append(np.concatenate([(o.state[p]["exp_avg"].double().numpy().reshape(-1) if p in o.state else np.zeros(p.numel())) for p in m.parameters()]))
        counts.append(float(next(iter(o.state.values()))["step"]) if o.state else 0.0)
    return np.asarray(losses, dtype=np.float64), ea, counts


def _train_models(pkg, spec, seed, p=0.2, head=(6,)):
    """[imposter, crew] from [(L, H)] x 2: one convolution stack, distinct recurrences."""
    return [make_model(pkg, N5, C3, 2, [3], [1], [1], 3, [1], L_, H, list(head), (5, 4)[t], seed + t, dropout=p) for t, (L_, H) in enumerate(spec)]


# (T, ((L, H) imposter, crew), head's hidden widths, layout).  The last case is the recurrence and head of notebooks/experiment.ipynb -- three
# layers of 64 (two 32-unit blocks: two waves at work per recurrence step), head [16, 16], T = 6 -- on the small convolution stack
TRAIN_CASES = [(2, ((3, 33), (2, 12)), (6,), "global"), (3, ((2, 33), (3, 12)), (6,), "perspective"), (6, ((3, 64), (3, 64)), (16, 16), "global")]


@pytest.mark.parametrize("T,spec,head,layout", TRAIN_CASES, ids=["T2-L3H33-L2H12-global", "T3-L2H33-L3H12-perspective", "T6-L3H64-notebook-global"])
def test_train_step_against_float64(pkg, env3, T, spec, head, layout):
    """torch autograd through the restatement in float64 with the library's own masks, online (net 0, p = 0.2) and target (net 1, p = 0.5)
    exported per (agent, team).  The project's tolerances: losses rtol 1e-4, Adam's exp_avg after the first step within 1e-4 of each
    tensor's max-abs, step counts exact.  Both teams train; 33 rows over a row tile of 32."""
    n = 33
    rng = np.random.default_rng(11 * T)
    models = _train_models(pkg, spec, seed=T, head=head)
    targets = _train_models(pkg, spec, seed=T + 50, head=head)
    batch = make_batch(rng, n, T, A3, C3, N5, 2, 4)
    if layout == "global":
        batch = as_global(batch)
    drops = _drops(pkg, 0.2, 0.5, offset=3)
    masks = _library_masks(pkg, env3, models, drops, n, T, A3)
    l64, ea64, st64 = masked_reference(pkg, models, targets, batch, 0.9, 1e-3, masks)
    l_plain, _, _ = masked_reference(pkg, models, targets, batch, 0.9, 1e-3, {})
    assert float(np.abs(l64 - l_plain).max()) > 1e-3 * float(np.abs(l_plain).max()), "the masks must matter for the comparison to say anything"
    losses, got = DropoutCall(pkg, env3, models, targets, batch, 0.9, drops).step()
    for t in range(2):
        assert got[t]["step"] == st64[t] and st64[t] >= 2.0, (t, got[t]["step"], st64[t])
        compare_tensors(models[t], got[t]["exp_avg"], ea64[t], ea64[t], f"team {t}")
    print(f"losses: kernel {losses}, float64 {l64}, rel {np.abs(losses - l64) / np.abs(l64)}; without masks {l_plain}")
    np.testing.assert_allclose(losses, l64, rtol=1e-4)


def test_train_step_with_an_empty_list(pkg, env3):
    """Agent 2 is never the imposter: the imposter team updates twice, the crew team three times; still the float64 result."""
    n, T = 33, 2
    rng = np.random.default_rng(61)
    models = _train_models(pkg, ((3, 12), (3, 12)), seed=9)
    batch = make_batch(rng, n, T, A3, C3, N5, 2, 4)
    batch["imposters"] = (np.arange(len(batch["imposters"])) % 2).astype(np.int16)
    drops = _drops(pkg, 0.2, 0.2)
    masks = _library_masks(pkg, env3, models, drops, n, T, A3)
    l64, ea64, st64 = masked_reference(pkg, models, models, batch, 0.9, 1e-3, masks)
    losses, got = DropoutCall(pkg, env3, models, models, batch, 0.9, drops).step()
    assert [got[0]["step"], got[1]["step"]] == st64 == [2.0, 3.0]
    for t in range(2):
        compare_tensors(models[t], got[t]["exp_avg"], ea64[t], ea64[t], f"team {t}")
    np.testing.assert_allclose(losses, l64, rtol=1e-4)


def _same_bits(a, b):
    return np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and all(
        np.array_equal(x.view(np.int32), y.view(np.int32)) for t in range(2) for x, y in zip(a[1][t]["bits"], b[1][t]["bits"]))


def test_train_step_bits(pkg, env3):
    """Bit for bit: two runs from equal state; an all-done batch under other target masks (y = r: the target network is not looked at); p = 0
    through the new entry against susnet_spatial_train_step; and what must differ does (other online masks, another offset)."""
    n, T = 33, 3
    rng = np.random.default_rng(62)
    models = _train_models(pkg, ((3, 33), (2, 12)), seed=13)
    targets = _train_models(pkg, ((3, 33), (2, 12)), seed=63)
    batch = make_batch(rng, n, T, A3, C3, N5, 2, 4)
    run = lambda b, drops, steps=2: [c.step() for c in [DropoutCall(pkg, env3, models, targets, b, 0.9, drops)] for _ in range(steps)][-1]
    a = run(batch, _drops(pkg, 0.2, 0.5))
    assert _same_bits(a, run(batch, _drops(pkg, 0.2, 0.5))), "two runs from equal state leave identical bytes"
    assert not _same_bits(a, run(batch, _drops(pkg, 0.2, 0.5, offset=1))), "the offset selects other masks"
    assert not _same_bits(a, run(batch, _drops(pkg, 0.2, 0.2))), "the target network's masks reach y where a row is not done"
    done = dict(batch, dones=np.ones_like(batch["dones"]))
    d = run(done, _drops(pkg, 0.2, 0.5))
    assert _same_bits(d, run(done, _drops(pkg, 0.2, 0.2))) and _same_bits(d, run(done, _drops(pkg, 0.2, 0.0)))
    assert not _same_bits(d, run(done, _drops(pkg, 0.5, 0.5)))
    plain_call = SpatialCall(pkg, env3, models, targets, batch, 0.9)
    plain = [plain_call.step() for _ in range(2)][-1]
    assert _same_bits(plain, run(batch, _drops(pkg, 0.0, 0.0))), "p = 0 through the new entry is susnet_spatial_train_step"
    assert not _same_bits(plain, a)


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------------------
def _notebook_like(pkg, env, seeds=(3, 4)):
    """The notebook's architecture at small widths on the Global featurizer's tensors of ``env``: rnn_layers 3, rnn_dropout 0.2."""
    _, planes, non = env._make_obs(pkg.ObsConfig("planes"), 1, rows=1)
    cfg = dict(input_image_size=planes.shape[-1], non_spatial_input_size=non.shape[-1] + env.n_agents, n_channels=[planes.shape[-3], 5, 3],
               strides=[1, 1], paddings=[1, 1], kernel_size=[3, 3], dilations=[1, 1], rnn_layers=3, rnn_hidden_dim=12, rnn_dropout=0.2,
               mlp_hidden_layer_dims=[8, 8])
    out = []
    for seed, n in zip(seeds, (env.n_imposter_actions, env.n_crew_actions)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            out.append(pkg.SpatialDQN(**cfg, n_actions=n).to(DEV))
    return out


def test_run_experiment_trains_under_dropout(pkg, tmp_path):
    """run_experiment on base_1v3, 16 envs, T = 2, rnn_layers 3, rnn_dropout 0.2, rnn_dropout_seed = 1: 7 ticks, a train step every 5.  The
    models act in eval mode (susnet_spatial_forward is the eval-mode forward) and learn under dropout on susnet_spatial_train_step_dropout:
    without the seed such a trainer takes torch_train_step, which leaves the models in training mode, and the next acting forward refuses
    them; with it the run completes on the device step, and the same call twice gives identical parameters."""
    raw8 = pkg.ObsConfig("raw", dtype=torch.uint8)
    mk_env = lambda: pkg.BatchedFourRoomEnv(1, 3, 5, batch=16, device=DEV, rng="philox", seed=7, auto_reset=True, grid_size=9, obs=raw8, max_time_steps=6)
    num_steps, k = 7, 5

    def run(base, **kw):
        env = mk_env()
        imp, crew = _notebook_like(pkg, env)
        imp.eval(), crew.eval()
        gen = torch.Generator(device=DEV)
        gen.manual_seed(5)
        metrics = pkg.run_experiment(env, num_steps=num_steps, imposter_model=imp, crew_model=crew, components=[], sequence_length=2,
                                     replay_buffer_size=500, replay_prepopulate_steps=4, batch_size=8, gamma=0.9, scheduler_time_steps=5,
                                     experiment_base_dir=base, learning_rate=1e-3, train_step_interval=k, target_update_interval=4,
                                     featurizer=pkg.GlobalFeaturizer(env), generator=gen, **kw)
        torch.cuda.synchronize()
        (run_dir,) = list(base.iterdir())
        return imp, crew, metrics, json.loads((run_dir / "config.json").read_text()), run_dir

    initial = _notebook_like(pkg, mk_env())
    imp, crew, metrics, config, run_dir = run(tmp_path / "a", rnn_dropout_seed=1)
    assert not imp.training and not crew.training  # (the device step does not touch the modules' mode: they go on acting in eval mode)
    assert config["train_step"] == "susnet_spatial_train_step" and config["rnn_dropout_seed"] == 1
    assert config["imposter_model_args"]["rnn_layers"] == 3 and config["imposter_model_args"]["rnn_dropout"] == 0.2
    m = metrics.metrics
    losses = m[pkg.SusMetrics.IMPOSTER_LOSS] + m[pkg.SusMetrics.CREW_LOSS]
    assert len(m[pkg.SusMetrics.IMPOSTER_LOSS]) == 1 + (num_steps - 1) // k and all(math.isfinite(v) and v > 0 for v in losses)
    for model, first in zip((imp, crew), initial):
        assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), first.parameters())), "the team trained"
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    written = sorted(p.name for p in run_dir.glob("imposter_spatial_dqn_*.pt"))
    assert "imposter_spatial_dqn_100%.pt" in written and "imposter_spatial_dqn_0.pt" in written and (run_dir / "crew_spatial_dqn_100%.pt").exists()
    # the same call twice: identical parameters and losses
    imp2, crew2, metrics2, _, _ = run(tmp_path / "b", rnn_dropout_seed=1)
    for a, b in ((imp, imp2), (crew, crew2)):
        assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert metrics2.metrics[pkg.SusMetrics.IMPOSTER_LOSS] == m[pkg.SusMetrics.IMPOSTER_LOSS]
    # another seed: other masks, other parameters; no seed: as before, the run does not get past its first train step
    imp3, _, _, _, _ = run(tmp_path / "c", rnn_dropout_seed=2)
    assert any(not torch.equal(p, q) for p, q in zip(imp.parameters(), imp3.parameters()))
    with pytest.raises(RuntimeError, match="training mode"):  # torch_train_step puts the models into training mode; the next acting forward refuses
        run(tmp_path / "d")
