"""The learner's half of the reference trainer on the device: ``DQNTeamTrainer.train_step`` (src/train.py:50-149) on a batch drawn
from a ``DeviceReplayBuffer`` (``ReplayBuffer.sample``, src/replay_memory.py:75-94).

* HIP path (``susnet_dqn_train_step``, csrc/susnet_train.h): reference ``MLP``s on a compiled-in feature layout (the layouts
  ``susnet_qnet_forward`` serves), a window of one state, one imposter.  The ring is read in place at the sampled indices; per (agent,
  team) update one gradient launch and one reduce + Adam launch, no host synchronisation, and the teams' packed images (what
  ``PolicyRollout`` acts with) are rewritten on the device.
* dense HIP path (``susnet_mlp_train_step``, csrc/susnet_mlp_train.h; opt-in: ``DeviceDQNTeamTrainer(..., dense=True)``): reference
  ``MLP``s of any served layer stack on ANY game and component set, one imposter, a window of T >= 1 states: the networks read the
  flattened window, ``T * F`` inputs (dqn.py:86-90), and T is the ring's ``trajectory_size``.  The batch's ``[n, T, S]`` windows are
  gathered and featurized as ``n * T`` rows (the FLAT featurizer kernel) into reused buffers -- ``[n * T, F]`` IS the ``[n][T * F]``
  layout the step reads --, then one call: the same launches per update, no host synchronisation.
  There is no packed image: a ``PolicyRollout(dense=True)`` reads the parameters in place and follows the step without a refresh.
  A ``DeviceDQNSweepTrainer`` over such trainers of one shape takes their steps in ONE call (``susnet_mlp_train_sweep``).
* spatial HIP path (``susnet_spatial_train_step``, csrc/susnet_spatial_train.h; opt-in: ``DeviceDQNTeamTrainer(..., spatial=True)``):
  reference ``SpatialDQN``s (CNN, tanh ``nn.RNN``, PReLU head) within ``susnet_spatial_forward``'s bounds on a ``GlobalFeaturizer`` or
  ``PerspectiveFeaturizer``, one imposter, no dropout between RNN layers.  The batch's windows and next windows are gathered and featurized
  into reused buffers, then one call: 1 + 4 launches per (agent, trained team), no host synchronisation.  A ``SpatialQNet`` of the same
  model reads the parameters in place and follows the step without a refresh.
* torch path (``torch_train_step``): the same algorithm in torch ops for anything else -- a ``SpatialDQN`` without ``spatial=True``, other
  layer stacks, longer windows, CPU tensors.

The parameters of each trained team live in ONE flat float32 buffer in ``model.parameters()`` order, and the modules' parameters are
views into it: after a step the ``nn.Module`` holds the new values (``dump_to_checkpoint`` works), whichever path ran.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib as L
from .policy import MLP, RandomEquiprobable, SpatialFeed, _weights_version, dense_stack, fill_spatial_net, linear_prelu_stack, spatial_desc, spatial_feed_mismatch

BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults (train.py:35-37 passes only lr)


def torch_train_step(models, targets, optimizers, gamma: float, state_feats, next_state_feats, actions, rewards, dones, imposters) -> List[float]:
    """``DQNTeamTrainer.train_step`` (train.py:50-149) on featurized batches: ``state_feats`` / ``next_state_feats`` = one
    ``(spatial, non_spatial)`` pair per agent (``generate_featurized_states()``), ``models`` / ``targets`` / ``optimizers`` = [imposter,
    crew] (an optimizer of None: the team does not train).  Returns ``[imposter_loss, crew_loss]`` summed over agents, as floats."""
    losses = [0.0, 0.0]
    if all(o is None for o in optimizers):
        return losses
    for opt in optimizers:  # train.py:64-67: ONCE per call -- the gradients accumulate over the agents
        if opt is not None:
            opt.zero_grad()
    if imposters.shape[1] != 1:
        raise ValueError("one imposter is served: the reference's train_step fails on two or more, `(batch.imposters == agent_idx).view(-1)` "
                         "(src/train.py:83) has n_imposters * N entries")
    for agent_idx, (sf, nf) in enumerate(zip(state_feats, next_state_feats)):
        imp_rows = (imposters == agent_idx).view(-1)
        for team, rows in ((0, imp_rows), (1, ~imp_rows)):
            opt, model, target = optimizers[team], models[team], targets[team]
            if opt is None or int(rows.sum()) == 0:
                continue
            model.train()
            q = model(sf[0][rows], sf[1][rows])
            values = torch.gather(q, 1, actions[rows, agent_idx].view(-1, 1)).view(-1)
            with torch.no_grad():
                done_mask = dones[rows].view(-1)
                r = rewards[rows, agent_idx].view(-1)
                y = r + gamma * torch.max(target(nf[0][rows], nf[1][rows]), dim=1)[0]
                y[done_mask] = r[done_mask]
            loss = F.mse_loss(values, y)
            loss.backward()
            losses[team] += loss.item()
            opt.step()
    return losses


def _flatten_into(module: nn.Module, device) -> torch.Tensor:
    """One flat float32 buffer holding ``module``'s parameters in ``parameters()`` order; the parameters become views into it."""
    params = list(module.parameters())
    flat = torch.cat([p.detach().reshape(-1).to(device, torch.float32) for p in params]) if params else torch.zeros(0, device=device)
    off = 0
    for p in params:
        n = p.numel()
        p.data = flat[off:off + n].view_as(p)
        off += n
    return flat


class DeviceDQNTeamTrainer:
    """``DQNTeamTrainer`` (train.py:40-149) with its models, target models (train.py:306-307, 341-343) and Adam optimizers
    (train.py:24-38), for a ``DeviceReplayBuffer`` of ``env``.  ``components``: the FlatFeaturizer components the networks read.
    ``policy``: a ``PolicyRollout`` whose fused images should follow the trained weights without a host re-pack (it must read the same
    ``components``).  ``featurizer``: what the torch path featurizes the ring's states with (``features.FlatFeaturizer`` over
    ``components`` by default; a ``SpatialDQN`` needs a ``GlobalFeaturizer`` / ``PerspectiveFeaturizer`` of the same env).
    ``dense=True`` (opt-in): what ``susnet_dqn_train_step`` does not serve goes to ``susnet_mlp_train_step`` where that serves it
    (``uses_dense``), before the torch path.  ``sequence_length``: the window length T the trained networks read (their input is
    ``T * F`` wide); None (default): T is taken from the networks' input width, ``dims[0] / F``.
    ``spatial=True`` (opt-in): trained ``SpatialDQN``s that ``susnet_spatial_train_step`` serves, with a Global or Perspective
    ``featurizer``, take that step (``uses_spatial``) -- after ``uses_hip`` and ``uses_dense``, before the torch path.
    ``rnn_dropout_seed`` (opt-in, with ``spatial=True``): ``SpatialDQN``s with ``rnn_dropout > 0`` between several RNN layers are served
    too, by ``susnet_spatial_train_step_dropout``: the online network always under dropout (``train_step`` puts it in training mode,
    train.py:104), the target network iff its module is in training mode (it is after ``create_copy()``, as in the reference); the masks
    are the library's (include/susnet.h), keyed by the seed and ``dropout_steps`` (the count of such steps: the next step's ``offset``).
    The two teams share seed and offset: an update's masks are drawn per (agent, batch row), and for one agent the teams' lists are
    disjoint rows of the batch (a row is the imposter's or the crew's), so no two updates of a step read the same mask elements."""

    def __init__(self, env, imposter_model: nn.Module, crew_model: Optional[nn.Module], components: Sequence[str], lr: float, gamma: float,
                 train_imposter: bool = True, train_crew: bool = True, policy=None, featurizer=None, dense: bool = False,
                 sequence_length: Optional[int] = None, spatial: bool = False, rnn_dropout_seed: Optional[int] = None):
        if env.n_imposters >= 2:
            raise ValueError("one imposter is served: the reference's train_step fails on two or more, `(batch.imposters == agent_idx).view(-1)` "
                             "(src/train.py:83) has n_imposters * N entries")
        self.env, self.components, self.lr, self.gamma, self.policy = env, list(components), float(lr), float(gamma), policy
        self.device = torch.device(env.device)
        self.models = [imposter_model, crew_model]
        # OptimizerType.build returns None for a random model (train.py:33-34)
        self.trained = [bool(flag) and m is not None and not isinstance(m, RandomEquiprobable) and any(True for _ in m.parameters())
                        for m, flag in ((imposter_model, train_imposter), (crew_model, train_crew))]
        self.targets: List[Optional[nn.Module]] = [None, None]
        self.flat: List[Optional[torch.Tensor]] = [None, None]
        self.target_flat: List[Optional[torch.Tensor]] = [None, None]
        self.exp_avg: List[Optional[torch.Tensor]] = [None, None]
        self.exp_avg_sq: List[Optional[torch.Tensor]] = [None, None]
        self.step_count: List[Optional[torch.Tensor]] = [None, None]
        for t, m in enumerate(self.models):
            if m is None:
                continue
            m.to(self.device)
            target = m.create_copy().to(self.device) if hasattr(m, "create_copy") else None
            self.targets[t] = target
            if self.trained[t]:
                self.flat[t] = _flatten_into(m, self.device)
                self.target_flat[t] = _flatten_into(target, self.device)
                self.exp_avg[t] = torch.zeros_like(self.flat[t])
                self.exp_avg_sq[t] = torch.zeros_like(self.flat[t])
                self.step_count[t] = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._optim: List[Optional[torch.optim.Adam]] = [None, None]
        # where each team's Adam state currently lives: "flat" (the buffers the kernels update) or "optim" (the torch optimizer)
        self._owner = ["flat", "flat"]
        self._dims = [self._mlp_dims(m) if tr else None for m, tr in zip(self.models, self.trained)]
        self.hip = (self.device.type == "cuda" and any(self.trained) and all(d is not None for d, tr in zip(self._dims, self.trained) if tr)
                    and self._served(self._io(), env.lib.susnet_dqn_workspace_bytes))
        if policy is not None and any(self._policy_image(t) is not None for t in range(2)) and list(policy.components) != self.components:
            raise ValueError(f"policy reads components {list(policy.components)}, the trainer {self.components}: the rewritten images would "
                             "belong to another feature layout")
        self._featurizer = featurizer
        self._ws, self._losses = None, None
        # the dense step: each trained team's [F, h.., n_actions] where susnet_mlp_train_step serves it
        stacks = [dense_stack(m) if tr else None for m, tr in zip(self.models, self.trained)]
        self._dense_dims = [s and s[2] for s in stacks]
        self.sequence_length = None if sequence_length is None else int(sequence_length)  # (the dense step's T: settled by _dense_served)
        self._gathered = None  # (n, T, gathered states, gathered next states, their featurized rows, the next states'): _gather
        self.dense = (bool(dense) and self.device.type == "cuda" and any(self.trained) and featurizer is None
                      and all(c in L.FLAT_COMPONENTS for c in self.components)
                      and all(d is not None for d, tr in zip(self._dense_dims, self.trained) if tr) and self._dense_served())
        # the spatial step: each trained team's SpatialDQN as susnet_spatial_train_step reads it
        self.rnn_dropout_seed = None if rnn_dropout_seed is None else int(rnn_dropout_seed) & (2**64 - 1)
        self.dropout_steps = 0
        self._spatial_nets = [self._spatial_net(m, dropout=self.rnn_dropout_seed is not None) if tr else None
                              for m, tr in zip(self.models, self.trained)]
        self.spatial = (bool(spatial) and self.device.type == "cuda" and any(self.trained) and self._spatial_featurizer() is not None
                        and all(d is not None for d, tr in zip(self._spatial_nets, self.trained) if tr) and self._spatial_served())

    # ---- configuration ----
    @staticmethod
    def _mlp_dims(model):
        """``[F, h1, .., h4, n_out]`` of a reference ``MLP`` of five Linear layers (what ``susnet_dqn_train_step`` may serve), or None."""
        if not isinstance(model, MLP):
            return None
        # Kept as it has been since the fused learner was written, and unlike every other caller of the recogniser: the widths are not asked
        # to chain, and a single-slope PReLU AFTER the fifth Linear is let through (make_mlp builds neither).  susnet_dqn_workspace_bytes sees
        # dims only, so such a module would still be taken for served: tightening this changes which trainers run on the HIP path
        stack = linear_prelu_stack(model.model, chained=False, trailing_act=True)
        return stack[2] if stack is not None and len(stack[0]) == 5 else None

    def _fill_team(self, tm, t: int, dims) -> None:
        """One trained team's ``susnet_dqn_team``: its stack, the Adam constants and the flat buffers the kernels update (the team's Adam
        state is brought back into them first, where the torch optimizer holds it)."""
        self._state_to_flat(t)
        tm.enabled, tm.n_dims = 1, len(dims)
        for i, v in enumerate(dims):
            tm.dims[i] = v
        tm.lr, tm.beta1, tm.beta2, tm.eps = self.lr, BETAS[0], BETAS[1], EPS
        tm.params, tm.target_params = self.flat[t].data_ptr(), self.target_flat[t].data_ptr()
        tm.exp_avg, tm.exp_avg_sq, tm.step = self.exp_avg[t].data_ptr(), self.exp_avg_sq[t].data_ptr(), self.step_count[t].data_ptr()

    def _io(self, ring=None, idx=None) -> "L.DqnIO":
        io = L.DqnIO()
        io.n_components = len(self.components)
        for i, c in enumerate(self.components):
            io.components[i] = L.FLAT_COMPONENTS[c]
        io.trajectory_size = ring.trajectory_size if ring is not None else 1
        io.gamma = self.gamma
        for t in range(2):
            tm = io.team[t]
            if not self.trained[t] or self._dims[t] is None:
                continue
            self._fill_team(tm, t, self._dims[t])  # (n_dims = 6: _mlp_dims)
            net = self._policy_image(t)
            tm.packed = net.packed.data_ptr() if net is not None else None
        if ring is not None:
            self._fill_ring(io, ring, idx)
        return io

    def _fill_ring(self, io, ring, idx=None) -> None:
        """``ring`` and the sampled ``idx`` into any learner's io: the three structs name these fields alike (``DqnIO`` reads the raw states
        in place as well)."""
        if isinstance(io, L.DqnIO):
            io.states, io.next_states = ring.states.data_ptr(), ring.next_states.data_ptr()
        io.actions, io.rewards = ring.actions.data_ptr(), ring.rewards.data_ptr()
        io.dones, io.imposters = ring.dones.data_ptr(), ring.imposters.data_ptr()
        io.max_size = ring.max_size
        if idx is not None:
            io.indices, io.n = idx.data_ptr(), idx.numel()

    def _served(self, io, workspace_bytes) -> bool:
        """Whether the library takes ``io`` -- a learner's io without ring or indices -- at ``max_size = n = 1``: ``workspace_bytes`` is the
        learner's own probe, which makes every check that reads no pointer."""
        io.max_size, io.n = 1, 1
        nbytes = C.c_uint64()
        return workspace_bytes(self.env._h, C.byref(io), C.byref(nbytes)) == 0

    def _policy_image(self, team):
        p = self.policy
        if p is None:
            return None
        # (a WindowedPolicyRollout has no packed image: SpatialQNet reads the parameters in place)
        if team == 0 and p.imposter_model is self.models[0]:
            return getattr(p, "fused_imposter", None)
        if team == 1 and p.crew_model is self.models[1]:
            return getattr(p, "fused_crew", None)
        return None

    def uses_hip(self, ring) -> bool:
        """Whether ``ring`` is trained on by ``susnet_dqn_train_step`` (else: the dense step where ``uses_dense``, else ``torch_train_step``)."""
        return self.hip and ring.trajectory_size == 1 and ring.states.device == self.device

    def uses_dense(self, ring) -> bool:
        """Whether ``ring`` is trained on by ``susnet_mlp_train_step``: a ``dense=True`` trainer of reference MLP stacks within the
        kernel's bounds whose input is the ring's window, ``trajectory_size * F`` wide, cuda tensors -- and ``uses_hip`` does not hold
        (that path goes first)."""
        return self.dense and not self.uses_hip(ring) and ring.trajectory_size == self.sequence_length and ring.states.device == self.device

    def _dense_io(self) -> "L.MlpTrainIO":
        io = L.MlpTrainIO()
        io.gamma = self.gamma
        for t in range(2):
            if self.trained[t] and self._dense_dims[t] is not None:
                self._fill_team(io.team[t], t, self._dense_dims[t])
        return io

    def _dense_served(self) -> bool:
        from .env import ObsConfig

        F = self.env._make_obs(ObsConfig("flat", self.components), 1, rows=1)[1].shape[-1]
        widths = set(d[0] for d, tr in zip(self._dense_dims, self.trained) if tr)
        T = self.sequence_length if self.sequence_length is not None else max(widths) // F
        if widths != {T * F} or not 1 <= T <= L.WINDOW_MAX_T or T * F > L.MLP_MAX_F:
            return False  # the networks do not read windows of this featurizer's rows
        self.sequence_length = T
        return self._served(self._dense_io(), self.env.lib.susnet_mlp_train_workspace_bytes)

    # ---- the spatial step's configuration ----
    def _spatial_featurizer(self):
        """"global" / the observation mode ("persp"; "persp_room" / "persp_room_mask" under partial observability) for a
        ``GlobalFeaturizer`` / ``PerspectiveFeaturizer`` of this env, else None."""
        from .features import GlobalFeaturizer, PerspectiveFeaturizer

        f = self._featurizer
        if isinstance(f, (GlobalFeaturizer, PerspectiveFeaturizer)) and f.env is self.env:
            return "global" if isinstance(f, GlobalFeaturizer) else f.config.mode
        return None

    def _spatial_net(self, model, dropout: bool = False):
        """``policy.spatial_desc`` of a ``SpatialDQN`` whose training-mode forward the kernels compute too -- the trainer's two own rules: no
        dropout between RNN layers (with ``dropout``: ``susnet_spatial_train_step_dropout`` computes it) and ``parameters()`` in the order of
        the flat layout the kernels assume (convolutions, RNN layer by layer, head) -- or None."""
        d = spatial_desc(model)
        if d is None or (d["p"] > 0 and not dropout):  # (nn.RNN drops out between layers in training mode: the plain kernels do not)
            return None
        names = [n for n, _ in model.named_parameters()]
        want = [f"cnn.model.{2 * l}.{w}" for l in range(len(d["convs"])) for w in ("weight", "bias")]
        want += [f"rnn.model.{w}_l{l}" for l in range(d["layers"]) for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        if names[:len(want)] != want or not all(n.startswith("prediction_head.") for n in names[len(want):]):
            return None
        return d

    def _spatial_dropout(self):
        """The two ``susnet_rnn_dropout`` ([imposter, crew]) of the next dropout step, or None where no trained team has dropout to apply."""
        if self.rnn_dropout_seed is None or not any(d is not None and d["p"] > 0 for d, tr in zip(self._spatial_nets, self.trained) if tr):
            return None
        drop = (L.RnnDropout * 2)()
        for t in range(2):
            d = self._spatial_nets[t]
            if self.trained[t] and d is not None:
                target = self.targets[t]
                drop[t].p[0] = d["p"]  # train_step: model.train() (train.py:104)
                drop[t].p[1] = d["p"] if target is not None and target.training else 0.0
            drop[t].seed, drop[t].offset, drop[t].row_base = self.rnn_dropout_seed, self.dropout_steps, 0
        return drop

    def _spatial_io(self, T: int) -> "L.SpatialTrainIO":
        io = L.SpatialTrainIO()
        io.gamma = self.gamma
        for t in range(2):
            d = self._spatial_nets[t]
            if not self.trained[t] or d is None:
                continue
            self._fill_team(io.team[t], t, d["dims"])
            fill_spatial_net(io.net[t], d, T)
        return io

    def _spatial_served(self) -> bool:
        env = self.env
        for t, n_actions in enumerate((env.n_imposter_actions, env.n_crew_actions)):
            if self.trained[t] and spatial_feed_mismatch(env, self._featurizer, self._spatial_nets[t], n_actions) is not None:
                return False  # the networks do not read this featurizer's tensors
        return self._served(self._spatial_io(1), env.lib.susnet_spatial_train_workspace_bytes)

    def uses_spatial(self, ring) -> bool:
        """Whether ``ring`` is trained on by ``susnet_spatial_train_step``: a ``spatial=True`` trainer of served ``SpatialDQN``s with a Global
        or Perspective featurizer, windows of at most ``SPATIAL_MAX_T`` states, cuda tensors -- and neither ``uses_hip`` nor ``uses_dense``
        holds (those paths go first)."""
        return (self.spatial and not self.uses_hip(ring) and not self.uses_dense(ring) and 1 <= ring.trajectory_size <= L.SPATIAL_MAX_T
                and ring.states.device == self.device)

    # ---- the train step ----
    def train_step(self, ring, batch_size: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """Sample ``batch_size`` ring rows uniformly with replacement (replay_memory.py:89) and take one train step.  Returns the
        device ``[2]`` losses ``[imposter, crew]`` (HIP path: without synchronising)."""
        assert ring.size > 0, "Replay buffer is empty, can't sample"
        idx = torch.randint(0, ring.size, (int(batch_size),), device=ring.states.device, generator=generator)
        return self.train_step_on_indices(ring, idx)

    def train_step_on_indices(self, ring, idx: torch.Tensor) -> torch.Tensor:
        idx = idx.to(ring.states.device, torch.int64).contiguous()
        if self.uses_hip(ring):
            return self._hip_step(ring, idx)
        if self.uses_dense(ring):
            return self._dense_step(ring, idx)
        if self.uses_spatial(ring):
            return self._spatial_step(ring, idx)
        return self._torch_step(ring, idx)

    def _workspace_and_losses(self, io, workspace_bytes) -> None:
        """``io.workspace`` (grown to what ``workspace_bytes`` -- the learner's own probe -- asks for this io) and ``io.losses_out``."""
        nbytes = C.c_uint64()
        L.check(workspace_bytes(self.env._h, C.byref(io), C.byref(nbytes)))
        if self._ws is None or self._ws.numel() < nbytes.value:
            self._ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        if self._losses is None:
            self._losses = torch.zeros(2, dtype=torch.float32, device=self.device)
        io.workspace, io.workspace_bytes = self._ws.data_ptr(), self._ws.numel()
        io.losses_out = self._losses.data_ptr()

    def _hip_io(self, ring, idx) -> "L.DqnIO":
        """The complete ``susnet_dqn_io`` of one step on ``ring`` at ``idx``: Adam state in the flat buffers, workspace and losses allocated."""
        io = self._io(ring, idx)
        self._workspace_and_losses(io, self.env.lib.susnet_dqn_workspace_bytes)
        return io

    def _hip_step(self, ring, idx):
        env = self.env
        io = self._hip_io(ring, idx)
        with torch.cuda.device(self.device):
            L.check(env.lib.susnet_dqn_train_step(env._h, C.byref(io), env._stream()))
        self._sync_policy_version()
        return self._losses.clone()  # (a new tensor per step, as the torch path returns; enqueued, no host wait)

    def _gather(self, ring, idx, make_rows):
        """The batch's ``[n, T, S]`` windows and next windows, gathered into buffers that are reused while ``(n, T)`` stays; ``make_rows()``
        builds what the step featurizes them into, once per pair of buffers.  Returns ``(windows, next windows, rows, next rows)``."""
        n, T = int(idx.numel()), ring.trajectory_size
        if self._gathered is None or self._gathered[:2] != (n, T):
            self._gathered = (n, T, torch.empty(n, *ring.states.shape[1:], dtype=ring.states.dtype, device=self.device),
                              torch.empty(n, *ring.next_states.shape[1:], dtype=ring.next_states.dtype, device=self.device),
                              make_rows(), make_rows())
        torch.index_select(ring.states, 0, idx, out=self._gathered[2])
        torch.index_select(ring.next_states, 0, idx, out=self._gathered[3])
        return self._gathered[2:]

    def _dense_prepare(self, ring, idx) -> "L.MlpTrainIO":
        """The dense step up to its launch: gather + featurize the batch's windows and next windows (``[n, T, S]``, as ``n * T`` rows) into
        reused buffers and fill the ``susnet_mlp_train_io`` on the ``[n][T * F]`` rows (workspace and losses allocated).  What
        ``_dense_step`` launches, and what a ``DeviceDQNSweepTrainer`` collects from every member before its one launch.  Nothing waits on
        the host (with ``env.check_errors`` the featurizer's row check is polled, as ``env.featurize`` does)."""
        from .env import ObsConfig

        env, n, T = self.env, int(idx.numel()), ring.trajectory_size
        io = self._dense_io()
        if n > 0:
            rows, next_rows, (spec, feat, _), (next_spec, next_feat, _) = self._gather(
                ring, idx, lambda: env._make_obs(ObsConfig("flat", self.components), 1, rows=n * T))
            io.feat, io.next_feat = feat.data_ptr(), next_feat.data_ptr()
        self._fill_ring(io, ring, idx)
        self._workspace_and_losses(io, env.lib.susnet_mlp_train_workspace_bytes)
        with torch.cuda.device(self.device):
            if n > 0:
                dt = env._ROW_DTYPES[rows.dtype]
                L.check(env.lib.susnet_featurize(env._h, rows.data_ptr(), dt, n * T, C.byref(spec), env._stream()))
                L.check(env.lib.susnet_featurize(env._h, next_rows.data_ptr(), dt, n * T, C.byref(next_spec), env._stream()))
                if env.check_errors:
                    env.poll_errors()
        return io

    def _dense_finish(self) -> None:
        """What follows a dense step's launch (the member's own, or a sweep's): a fused image of the trained weights is re-packed."""
        if self.policy is not None and any(self._policy_image(t) is not None for t in range(2)):
            self.policy.refresh_weights(force=True)  # (a fused image of these weights: only where the fused step was switched off by hand)

    def _dense_step(self, ring, idx):
        """``_dense_prepare``, then ``susnet_mlp_train_step`` on the rows where they lie."""
        env = self.env
        io = self._dense_prepare(ring, idx)
        with torch.cuda.device(self.device):
            L.check(env.lib.susnet_mlp_train_step(env._h, C.byref(io), env._stream()))
        self._dense_finish()
        return self._losses.clone()

    def _spatial_prepare(self, ring, idx):
        """The spatial step up to its launch: gather the batch's ``[n, T, S]`` windows and next windows and featurize them (two
        ``policy.SpatialFeed``s: ``n * T`` rows each, the featurizer's kernel, reused buffers), fill the ``susnet_spatial_train_io`` (workspace
        and losses allocated) and the two ``susnet_rnn_dropout`` of the step (None: the plain step).  Returns ``(io, drop)``: what
        ``_spatial_step`` launches, and what a ``DeviceDQNSweepTrainer`` collects from every member before its one launch.  Nothing waits
        on the host (with ``env.check_errors`` the featurizer's row check is polled)."""
        env, n, T, A = self.env, int(idx.numel()), ring.trajectory_size, self.env.n_agents
        io = self._spatial_io(T)
        if n > 0:
            rows, next_rows, feed, next_feed = self._gather(ring, idx, lambda: SpatialFeed(env, self._featurizer, n, T))
            io.spatial, io.next_spatial = feed.spatial.data_ptr(), next_feed.spatial.data_ptr()
            io.non_spatial, io.next_non_spatial = feed.non_spatial.data_ptr(), next_feed.non_spatial.data_ptr()
            sp, ns = feed.strides(A)
            for d in range(3):
                io.spatial_stride[d], io.non_spatial_stride[d] = sp[d], ns[d]
        self._fill_ring(io, ring, idx)
        drop = self._spatial_dropout()
        self._workspace_and_losses(io, env.lib.susnet_spatial_train_workspace_bytes if drop is None
                                   else env.lib.susnet_spatial_train_dropout_workspace_bytes)
        with torch.cuda.device(self.device):
            if n > 0:
                feed.featurize(rows)
                next_feed.featurize(next_rows)
                if env.check_errors:
                    env.poll_errors()
                feed.finish()
                next_feed.finish()
        return io, drop

    def _spatial_step(self, ring, idx):
        """``_spatial_prepare``, then ``susnet_spatial_train_step`` (with dropout structs: ``susnet_spatial_train_step_dropout``) on the
        tensors where they lie."""
        env = self.env
        io, drop = self._spatial_prepare(ring, idx)
        with torch.cuda.device(self.device):
            if drop is None:
                L.check(env.lib.susnet_spatial_train_step(env._h, C.byref(io), env._stream()))
            else:
                L.check(env.lib.susnet_spatial_train_step_dropout(env._h, C.byref(io), drop, env._stream()))
                self.dropout_steps += 1  # (after the check: a refused call does not use up an offset)
        return self._losses.clone()

    def _sync_policy_version(self):
        p = self.policy
        if p is not None and any(self._policy_image(t) is not None for t in range(2)):
            # the images were rewritten on the device (in-place kernel writes leave the parameters' versions as they were)
            p._packed_version = (_weights_version(p.imposter_model), _weights_version(p.crew_model))

    def optimizers(self):
        """torch.optim.Adam per team over the module parameters (the torch path), state mirrored from the flat buffers."""
        for t in range(2):
            if self.trained[t] and self._optim[t] is None:
                self._optim[t] = torch.optim.Adam(self.models[t].parameters(), lr=self.lr)
        return self._optim

    def _torch_step(self, ring, idx):
        from .features import FlatFeaturizer

        opts = self.optimizers()
        for t in range(2):
            if self.trained[t] and self._owner[t] == "flat":
                self._optim[t].load_state_dict(self._flat_state_dict(t))
                self._owner[t] = "optim"
        if self._featurizer is None:
            self._featurizer = FlatFeaturizer(self.env, self.components)
        fz = self._featurizer
        fz.fit(ring.states[idx])
        sf = fz.generate_featurized_states()
        fz.fit(ring.next_states[idx])
        nf = fz.generate_featurized_states()
        losses = torch_train_step(self.models, self.targets, [o if tr else None for o, tr in zip(opts, self.trained)], self.gamma, sf, nf,
                                  ring.actions[idx], ring.rewards[idx], ring.dones[idx], ring.imposters[idx])
        if self.policy is not None:
            self.policy.refresh_weights(force=True)
        return torch.tensor(losses, dtype=torch.float32, device=self.device)

    # ---- optimizer state, in torch.optim.Adam's format ----
    def _state_to_flat(self, t):
        if self.trained[t] and self._owner[t] == "optim":
            self._set_state(t, self._optim[t].state_dict())
            self._owner[t] = "flat"

    def state_tensors(self, team: int):
        """``(exp_avg, exp_avg_sq, step)`` of ``team`` as flat device tensors in ``parameters()`` order."""
        self._state_to_flat(team)
        return self.exp_avg[team], self.exp_avg_sq[team], self.step_count[team]

    def optimizer_state_dict(self, team: int) -> dict:
        """``torch.optim.Adam(model.parameters(), lr).state_dict()`` of ``team`` (0 imposter, 1 crew)."""
        assert self.trained[team], "this team has no optimizer"
        if self._owner[team] == "optim":
            return self._optim[team].state_dict()
        return self._flat_state_dict(team)

    def _flat_state_dict(self, team: int) -> dict:
        params = list(self.models[team].parameters())
        state = {}
        step = float(self.step_count[team].item())
        if step > 0:
            off = 0
            for i, p in enumerate(params):
                n = p.numel()
                state[i] = {"step": torch.tensor(step), "exp_avg": self.exp_avg[team][off:off + n].view_as(p).clone(),
                            "exp_avg_sq": self.exp_avg_sq[team][off:off + n].view_as(p).clone()}
                off += n
        group = {"lr": self.lr, "betas": BETAS, "eps": EPS, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
                 "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, team: int, sd: dict) -> None:
        assert self.trained[team], "this team has no optimizer"
        self._set_state(team, sd)
        self._owner[team] = "flat"

    def _set_state(self, team, sd):
        params = list(self.models[team].parameters())
        st = sd["state"]
        off, step = 0, 0.0
        for i, p in enumerate(params):
            n = p.numel()
            s = st.get(i)
            if s:
                self.exp_avg[team][off:off + n].copy_(s["exp_avg"].reshape(-1))
                self.exp_avg_sq[team][off:off + n].copy_(s["exp_avg_sq"].reshape(-1))
                step = float(s["step"])
            else:
                self.exp_avg[team][off:off + n].zero_()
                self.exp_avg_sq[team][off:off + n].zero_()
            off += n
        self.step_count[team].fill_(step)

    # ---- snapshot / restore ----
    @staticmethod
    def _module_tensors(module) -> dict:
        return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}

    @staticmethod
    @torch.no_grad()
    def _load_module_tensors(module, tensors: dict, who: str) -> None:
        """``tensors`` into ``module``'s parameters and buffers IN PLACE (``copy_`` into the storage they have: views stay views)."""
        own = module.state_dict()
        if list(own) != list(tensors):
            raise ValueError(f"load_state_dict: the {who} was saved with the entries {list(tensors)}, this module has {list(own)}")
        for k, v in own.items():
            if tuple(v.shape) != tuple(tensors[k].shape):
                raise ValueError(f"load_state_dict: {who}: {k} was saved as {tuple(tensors[k].shape)}, this module's is {tuple(v.shape)}")
            v.copy_(tensors[k])

    def state_dict(self) -> dict:
        """The learner between two train steps, as host tensors and plain values.  Per team with a model: whether it trains, the modules'
        train / eval mode (model and target); of a trained team the online and target parameters (``flat``, ``target_flat``), the Adam
        moments and ``step_count`` as the flat buffers hold them, which side owns the Adam state (``_owner``) and -- where that is the
        torch optimizer -- its ``state_dict`` (``optimizer_state_dict``); of a team that acts without training the modules' own tensors,
        so that a run restored into fresh models acts with the saved ones.  Plus ``dropout_steps``.  Synchronises."""
        teams = []
        for t, m in enumerate(self.models):
            if m is None:
                teams.append(None)
                continue
            target = self.targets[t]
            team = {"trained": self.trained[t], "training": bool(m.training), "target_training": None if target is None else bool(target.training)}
            if self.trained[t]:
                team.update(flat=self.flat[t].cpu(), target_flat=self.target_flat[t].cpu(), exp_avg=self.exp_avg[t].cpu(),
                            exp_avg_sq=self.exp_avg_sq[t].cpu(), step_count=self.step_count[t].cpu(), owner=self._owner[t],
                            optimizer=self.optimizer_state_dict(t) if self._owner[t] == "optim" else None)
                if team["optimizer"] is not None:
                    team["optimizer"] = {"state": {i: {k: v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v for k, v in s.items()}
                                                   for i, s in team["optimizer"]["state"].items()},
                                         "param_groups": team["optimizer"]["param_groups"]}
            else:
                team.update(model=self._module_tensors(m), target=None if target is None else self._module_tensors(target))
            teams.append(team)
        return {"teams": teams, "dropout_steps": int(self.dropout_steps), "lr": self.lr, "gamma": self.gamma,
                "rnn_dropout_seed": self.rnn_dropout_seed}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """Restore ``state_dict()``'s learner into this one, built over models of the same shapes with the same ``lr``, ``gamma``,
        ``train_*`` flags and ``rnn_dropout_seed`` (a difference is a ``ValueError`` that names it).  Everything is written into the
        existing flat buffers IN PLACE: the modules' parameters stay views of them, a policy that reads the parameters in place follows,
        and one that acts from packed images re-packs them (``policy.refresh_weights(force=True)``, where the trainer was built with its
        policy).  Where the torch optimizer owned the Adam state it owns it again, with the saved ``state_dict``."""
        for k in ("lr", "gamma", "rnn_dropout_seed"):
            if sd[k] != getattr(self, k):
                raise ValueError(f"load_state_dict: the trainer was saved with {k} = {sd[k]!r}, this one has {getattr(self, k)!r}")
        for t, (m, team) in enumerate(zip(self.models, sd["teams"])):
            name = ("imposter", "crew")[t]
            if (m is None) != (team is None):
                raise ValueError(f"load_state_dict: the {name} team had {'no' if team is None else 'a'} model when the trainer was saved, "
                                 f"this one has {'none' if m is None else 'one'}")
            if m is None:
                continue
            if bool(team["trained"]) != self.trained[t]:
                raise ValueError(f"load_state_dict: the {name} team was saved with trained = {team['trained']}, this one has {self.trained[t]}")
            if self.trained[t] and team["flat"].numel() != self.flat[t].numel():
                raise ValueError(f"load_state_dict: the {name} model was saved with {team['flat'].numel()} parameters, this one has "
                                 f"{self.flat[t].numel()}")
        for t, (m, team) in enumerate(zip(self.models, sd["teams"])):
            if m is None:
                continue
            target = self.targets[t]
            if self.trained[t]:
                for key in ("flat", "target_flat", "exp_avg", "exp_avg_sq", "step_count"):
                    getattr(self, key)[t].copy_(team[key])
                self._owner[t] = "flat"
                if team["owner"] == "optim":  # the torch optimizer holds the state again, as saved (its tensors on the parameters' device)
                    self.optimizers()[t].load_state_dict(team["optimizer"])
                    self._owner[t] = "optim"
            else:
                self._load_module_tensors(m, team["model"], f"{('imposter', 'crew')[t]} model")
                if target is not None and team["target"] is not None:
                    self._load_module_tensors(target, team["target"], f"{('imposter', 'crew')[t]} target model")
            m.train(bool(team["training"]))
            if target is not None and team["target_training"] is not None:
                target.train(bool(team["target_training"]))
        self.dropout_steps = int(sd["dropout_steps"])
        if self.policy is not None:
            self.policy.refresh_weights(force=True)

    # ---- target networks ----
    @torch.no_grad()
    def sync_targets(self) -> None:
        """``target.load_state_dict(model.state_dict())`` for both teams (train.py:341-343)."""
        for t in range(2):
            if self.targets[t] is None:
                continue
            if self.target_flat[t] is not None:
                self.target_flat[t].copy_(self.flat[t])
            else:
                self.targets[t].load_state_dict(self.models[t].state_dict())


def sweep_chunks(n_members: int, limit: int = L.DQN_MAX_LEARNERS):
    """``[(lo, hi), ...]``: the members of a sweep in order, in calls of at most ``limit`` (``SUSNET_DQN_MAX_LEARNERS``) learners."""
    return [(lo, min(lo + limit, n_members)) for lo in range(0, n_members, limit)]


class DeviceDQNSweepTrainer:
    """The train steps of a sweep -- the reference's loops over ``run_experiment(**config)`` (notebooks/experiment_1v1.ipynb,
    notebooks/experiment_mlp.ipynb: one game, one model shape, gamma 0.99 / 0.9 / 0.8) -- taken in lockstep: ``trainers`` are independent
    ``DeviceDQNTeamTrainer`` objects, each over its own env, models and policy, and one ``train_step`` steps every one of them.

    When every member is served by the HIP path and the members have one shape (``compatible()``), the step is ONE
    ``susnet_dqn_train_sweep`` call per chunk of at most 16 members: the launches of one learner's step with the learner as the grid's
    second dimension, each member's result bitwise what its own ``train_step_on_indices`` leaves.  When every member takes the spatial
    step (``DeviceDQNTeamTrainer(spatial=True)`` over served ``SpatialDQN``s: ``uses_spatial``) on windows of one length, the members
    have one shape and the index counts agree, every member prepares its own batch (gather, featurize: ``_spatial_prepare``) and the step
    is ONE ``susnet_spatial_train_sweep`` call per chunk of at most ``SPATIAL_SWEEP_MAX_LEARNERS`` members, again bitwise each member's
    own step, dropout masks included (a member's ``dropout_steps`` advances as its own steps would advance it).  The trainer owns the
    call's table buffer and the ``[K, 2]`` losses.  When every member takes the dense step (``DeviceDQNTeamTrainer(dense=True)`` over
    served MLP stacks: ``uses_dense``) on windows of one length, with one shape and equal index counts, every member prepares its own
    batch (gather, featurize: ``_dense_prepare``) and the step is ONE ``susnet_mlp_train_sweep`` call per chunk of at most
    ``MLP_SWEEP_MAX_LEARNERS`` members, bitwise each member's own step; a member's fused image of the trained weights, where one
    exists, is re-packed behind it as the member's own step does.  The order is: fused sweep, spatial sweep, dense sweep.  Otherwise
    the members' own ``train_step_on_indices`` run one after another (the torch path for CPU tensors and anything else unserved)."""

    def __init__(self, trainers: Sequence[DeviceDQNTeamTrainer]):
        self.trainers = list(trainers)
        if not self.trainers:
            raise ValueError("a sweep needs at least one trainer")
        if len(set(id(t) for t in self.trainers)) != len(self.trainers):
            raise ValueError("a trainer appears twice in the sweep: two learners would update the same parameters")
        self._losses = None
        self._table = None  # susnet_spatial_train_sweep's device table

    def __len__(self):
        return len(self.trainers)

    @staticmethod
    def _spatial_shape(t: DeviceDQNTeamTrainer):
        """What ``susnet_spatial_train_sweep`` requires its learners to agree on beyond the env, of a ``spatial=True`` trainer: the
        featurizer's layout, each trained team's network (the dropout probability itself may differ) and whether the team is masked (a
        p > 0 between several RNN layers, with a dropout seed), and whether the step passes dropout structs at all.  None otherwise."""
        if not t.spatial:
            return None
        nets = [None if not tr or d is None else
                ([d[key] for key in ("N", "C", "Fn", "k", "convs", "layers", "hidden", "dims")],
                 t.rnn_dropout_seed is not None and d["p"] > 0 and d["layers"] > 1)
                for d, tr in zip(t._spatial_nets, t.trained)]
        return t._spatial_featurizer(), nets, t._spatial_dropout() is None

    @staticmethod
    def _dense_shape(t: DeviceDQNTeamTrainer):
        """What ``susnet_mlp_train_sweep`` requires its learners to agree on beyond the env, of a ``dense=True`` trainer: each trained
        team's layer stack ``[T * F, h.., n_actions]`` and the window length T.  None otherwise."""
        if not getattr(t, "dense", False):
            return None
        return t._dense_dims, t.sequence_length

    def compatible(self) -> bool:
        """Whether the members agree on what shapes the step (what ``susnet_dqn_train_sweep``, ``susnet_spatial_train_sweep`` and
        ``susnet_mlp_train_sweep`` require): device, agent and imposter count, raw row size, grid, components, which teams train and their
        layer dims; of ``spatial=True`` members also the featurizer's layout, the networks and which teams are under a dropout mask
        (``_spatial_shape``); of two ``dense=True`` members also the dense stacks and the window length (``_dense_shape``; a member
        without ``dense`` never takes the dense step, so it constrains nothing there).  gamma, learning rate, weights, and the dropout
        probability and seed may differ."""
        a = self.trainers[0]
        for b in self.trainers[1:]:
            ea, eb = a.env, b.env
            if (b.device != a.device or eb.n_agents != ea.n_agents or eb.n_imposters != ea.n_imposters
                    or eb.flattened_state_size != ea.flattened_state_size or eb.grid.shape != ea.grid.shape or not (eb.grid == ea.grid).all()
                    or b.components != a.components or b.trained != a.trained or b._dims != a._dims
                    or self._spatial_shape(b) != self._spatial_shape(a)):
                return False
            da, db = self._dense_shape(a), self._dense_shape(b)
            if da is not None and db is not None and da != db:
                return False
        return True

    def uses_hip(self, rings) -> bool:
        """Whether a step on ``rings`` (one per member) is served by ``susnet_dqn_train_sweep`` for ALL members (else: the per-member loop)."""
        return len(rings) == len(self.trainers) and all(t.uses_hip(r) for t, r in zip(self.trainers, rings)) and self.compatible()

    def uses_spatial(self, rings) -> bool:
        """Whether a step on ``rings`` (one per member) is served by ``susnet_spatial_train_sweep`` for ALL members: every member takes
        the spatial step on its ring, the rings' windows have one length, and the members have one shape (else: the per-member loop)."""
        return (len(rings) == len(self.trainers) and all(t.uses_spatial(r) for t, r in zip(self.trainers, rings))
                and len(set(r.trajectory_size for r in rings)) == 1 and self.compatible())

    def uses_dense(self, rings) -> bool:
        """Whether a step on ``rings`` (one per member) is served by ``susnet_mlp_train_sweep`` for ALL members: every member takes the
        dense step on its ring, the rings' windows have one length, and the members have one shape (else: the per-member loop)."""
        return (len(rings) == len(self.trainers) and all(t.uses_dense(r) for t, r in zip(self.trainers, rings))
                and len(set(r.trajectory_size for r in rings)) == 1 and self.compatible())

    def train_step(self, rings, batch_size: int, generators=None) -> torch.Tensor:
        """Draw each member's ``batch_size`` ring rows with its own generator -- the draw the member's ``train_step`` makes -- and take
        one sweep step.  Returns the device ``[K, 2]`` losses."""
        generators = list(generators) if generators is not None else [None] * len(self.trainers)
        idxs = []
        for ring, g in zip(rings, generators):
            assert ring.size > 0, "Replay buffer is empty, can't sample"
            idxs.append(torch.randint(0, ring.size, (int(batch_size),), device=ring.states.device, generator=g))
        return self.train_step_on_indices(rings, idxs)

    def train_step_on_indices(self, rings, idxs) -> torch.Tensor:
        """One train step of every member on its own ring at its own indices.  Returns the device ``[K, 2]`` losses ``[imposter, crew]``
        per member (HIP path: without synchronising)."""
        K = len(self.trainers)
        if len(rings) != K or len(idxs) != K:
            raise ValueError(f"a sweep of {K} members needs {K} rings and {K} index tensors")
        idxs = [i.to(r.states.device, torch.int64).contiguous() for r, i in zip(rings, idxs)]
        same_n = len(set(int(i.numel()) for i in idxs)) == 1
        if same_n and not self.uses_hip(rings) and self.uses_spatial(rings):
            return self._spatial_sweep_step(rings, idxs)
        if same_n and not self.uses_hip(rings) and self.uses_dense(rings):
            return self._dense_sweep_step(rings, idxs)
        if not (self.uses_hip(rings) and same_n):
            return torch.stack([t.train_step_on_indices(r, i) for t, r, i in zip(self.trainers, rings, idxs)])
        first = self.trainers[0]
        lib, stream = first.env.lib, first.env._stream
        out = self._chunked_step(L.DQN_MAX_LEARNERS, L.DqnIO, lambda k: (self.trainers[k]._hip_io(rings[k], idxs[k]), None),
                                 lambda envs, ios, drops, n: lib.susnet_dqn_train_sweep(envs, ios, n, stream()))
        for t in self.trainers:
            t._sync_policy_version()
        return out

    def _spatial_sweep_step(self, rings, idxs) -> torch.Tensor:
        """Every member's ``_spatial_prepare``, then one ``susnet_spatial_train_sweep`` per chunk of ``SPATIAL_SWEEP_MAX_LEARNERS``."""
        first = self.trainers[0]
        lib, stream = first.env.lib, first.env._stream
        if self._table is None:
            nbytes = C.c_uint64()
            L.check(lib.susnet_spatial_train_sweep_table_bytes(L.SPATIAL_SWEEP_MAX_LEARNERS, C.byref(nbytes)))
            self._table = torch.empty(int(nbytes.value), dtype=torch.uint8, device=first.device)
        table = self._table
        return self._chunked_step(L.SPATIAL_SWEEP_MAX_LEARNERS, L.SpatialTrainIO, lambda k: self.trainers[k]._spatial_prepare(rings[k], idxs[k]),
                                  lambda envs, ios, drops, n: lib.susnet_spatial_train_sweep(envs, ios, drops, n, table.data_ptr(), table.numel(),
                                                                                             stream()))

    def _dense_sweep_step(self, rings, idxs) -> torch.Tensor:
        """Every member's ``_dense_prepare``, then one ``susnet_mlp_train_sweep`` per chunk of ``MLP_SWEEP_MAX_LEARNERS``; behind it every
        member's ``_dense_finish``, as its own step ends."""
        first = self.trainers[0]
        lib, stream = first.env.lib, first.env._stream
        out = self._chunked_step(L.MLP_SWEEP_MAX_LEARNERS, L.MlpTrainIO, lambda k: (self.trainers[k]._dense_prepare(rings[k], idxs[k]), None),
                                 lambda envs, ios, drops, n: lib.susnet_mlp_train_sweep(envs, ios, n, stream()))
        for t in self.trainers:
            t._dense_finish()
        return out

    def _chunked_step(self, limit: int, io_type, prepare, call) -> torch.Tensor:
        """The members' steps in library calls of at most ``limit`` learners each.  ``prepare(k)``: member k's complete io and its two dropout
        structs (or None) -- compatible(): all members pass them, or none does --; its losses go to row k of the trainer's ``[K, 2]``
        tensor.  ``call(envs, ios, drops, n)``: the library call on one chunk.  A chunk's members that passed dropout structs advance their
        ``dropout_steps`` after the checked call, as a member's own step does: a refused call uses up no offset."""
        K, first = len(self.trainers), self.trainers[0]
        if self._losses is None or self._losses.shape[0] != K:
            self._losses = torch.zeros(K, 2, dtype=torch.float32, device=first.device)
        row_bytes = self._losses.stride(0) * self._losses.element_size()
        for lo, hi in sweep_chunks(K, limit):
            n = hi - lo
            ios, envs, drops = (io_type * n)(), (C.c_void_p * n)(), None
            for j, k in enumerate(range(lo, hi)):
                io, drop = prepare(k)
                io.losses_out = self._losses.data_ptr() + k * row_bytes
                ios[j], envs[j] = io, self.trainers[k].env._h
                if drop is not None:
                    drops = drops if drops is not None else (L.RnnDropout * (2 * n))()
                    drops[2 * j], drops[2 * j + 1] = drop[0], drop[1]
            with torch.cuda.device(first.device):
                L.check(call(envs, ios, drops, n))
            if drops is not None:
                for k in range(lo, hi):
                    self.trainers[k].dropout_steps += 1
        return self._losses.clone()

    @torch.no_grad()
    def sync_targets(self) -> None:
        for t in self.trainers:
            t.sync_targets()
