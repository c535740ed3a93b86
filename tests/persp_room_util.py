"""Shared by the room-masked Perspective tests (test_persp_room_host.py, test_gpu_persp_room*.py): the reference-pinned fixture
(tests/golden/generate_persp_room.py -> tests/golden/persp_room/*.npz), random raw rows of any game, and a featurizer object whose tensors
are the HOST restatement ``features.room_mask_views`` -- what the torch module and ``torch_train_step`` are run on."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_DIR = os.path.join(ROOT, "tests", "golden", "persp_room")
FIXTURES = ("base_1v2_j4", "tagging_1v4_j5")


def load_fixture(name):
    d = np.load(os.path.join(FIXTURE_DIR, name + ".npz"))
    return json.loads(str(d["meta"])), {k: d[k] for k in d.files if k != "meta"}


class ShapeEnv:
    """What ``features.room_mask_views`` reads of an env, for the tests that have no device."""

    def __init__(self, n_agents, n_jobs, n):
        self.n_agents, self.n_jobs, self.n_rows = n_agents, n_jobs, n


def random_rows(rng, n_rows, A, J, N, tagging, dead=0.3):
    """uint8 raw rows (``flatten_state`` order) with every field drawn independently: cells anywhere on the N x N grid -- walls included,
    the featurizers do not look at the wall map --, agents dead with probability ``dead``, jobs done or not, small tag counts."""
    parts = [rng.integers(0, N, (n_rows, 2 * A)), rng.random((n_rows, A)) >= dead, rng.integers(0, N, (n_rows, 2 * J)), rng.random((n_rows, J)) < 0.5]
    if tagging:
        parts += [rng.random((n_rows, A)) < 0.5, rng.integers(0, A, (n_rows, A)), rng.integers(1, 7, (n_rows, 1))]
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts], axis=1)


def fixture_cases(rows, A, J):
    """The cases the issue lists, asserted on the stored rows (N = 9) as the generator asserted them."""
    room = lambda x, y: (x <= 4) + 2 * (y <= 4)
    rows = rows.astype(np.int64)
    pos, alive = rows[:, :2 * A].reshape(-1, A, 2), rows[:, 2 * A:3 * A] != 0
    jobs, done = rows[:, 3 * A:3 * A + 2 * J].reshape(-1, J, 2), rows[:, 3 * A + 2 * J:3 * A + 3 * J] != 0
    rooms, jroom = room(pos[..., 0], pos[..., 1]), room(jobs[..., 0], jobs[..., 1])
    assert set(np.unique(rooms)) == {0, 1, 2, 3}, "an observer in each of the four rooms"
    for axis, v in ((0, 4), (1, 4), (0, 5), (1, 5)):
        assert (pos[..., axis] == v).any(), f"an observer at coordinate {axis} = {v}"
    same, other = rooms[:, :, None] == rooms[:, None, :], ~np.eye(A, dtype=bool)[None]
    assert (same & other & alive[:, None, :]).any() and (~same & alive[:, None, :]).any(), "a living agent inside and one outside the observer's room"
    assert (~alive).any(), "a dead observer"
    assert (same & other & ~alive[:, None, :]).any(), "a dead agent inside the observer's room"
    jsame = rooms[:, :, None] == jroom[:, None, :]
    for inside in (True, False):
        for d in (True, False):
            assert ((jsame == inside) & (done[:, None, :] == d)).any(), f"a job inside={inside} done={d}"


class HostRoomFeaturizer:
    """``PerspectiveFeaturizer(env, partially_observable=True, ...)``'s interface over ``features.room_mask_views``: float32 device
    tensors of the host restatement.  Not a PerspectiveFeaturizer, so nothing routes it to the kernels."""

    def __init__(self, pkg, env, add_mask=True):
        self.pkg, self.env, self.add_mask = pkg, env, add_mask
        self.spatial = self.non_spatial = None

    def fit(self, state_sequence):
        sp, non = self.pkg.features.room_mask_views(self.env, state_sequence, self.add_mask)
        self.spatial = torch.from_numpy(sp).to(self.env.device, torch.float32)
        self.non_spatial = torch.from_numpy(non).to(self.env.device, torch.float32)

    def generate_featurized_states(self):
        return [(self.spatial[:, :, i], self.non_spatial[:, :, i]) for i in range(self.env.n_agents)]


NET = dict(strides=[1, 1], paddings=[1, 1], kernel_size=[3, 3], dilations=[1, 1], rnn_layers=1, rnn_hidden_dim=16, rnn_dropout=0.0, mlp_hidden_layer_dims=[12])
ACTING_SEEDS = (3, 4)  # (test_persp_room_host.py checks them: the torch modules alone have few near-ties on the fixture's windows)


def acting_models(pkg, A, N, Fn, n_imposter_actions, n_crew_actions, device, seeds=ACTING_SEEDS, mask=True):
    """Small seeded ``SpatialDQN``s on the room-masked views: ``n_channels = [A + 3, 4, 3]`` (A + 2 without the mask channel), two 3 x 3
    convolutions, one RNN layer of 16, one hidden layer of 12; (imposter, crew), in eval mode."""
    out = []
    for seed, n in zip(seeds, (n_imposter_actions, n_crew_actions)):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            out.append(pkg.SpatialDQN(**NET, input_image_size=N, non_spatial_input_size=Fn, n_channels=[A + (3 if mask else 2), 4, 3],
                                      n_actions=n).to(device).eval())
    return out
