"""CPU-only: the ONE statement of what a served SpatialDQN is, held to what its copies answered before they were merged.  In C the spatial
rules (``check_spatial_net`` / ``check_spatial_head``, csrc/susnet_host.h) serve ``susnet_spatial_forward`` and the SpatialDQN learner, and
the handle / Adam / pointer / workspace checks serve the dense and the spatial learner; in Python ``policy.spatial_desc`` serves
``SpatialQNet`` and the trainer, ``policy.spatial_feed_mismatch`` the actor, the trainer and ``spatial_unserved_reason``.
tests/golden/spatial_refusals.json holds the answers of the code before the merge (tests/golden/generate_spatial_refusals.py, run there) to
the tables of tests/spatial_desc_cases.py: every refusal's return code and full message, the wrappers' accept sets, the reasons' texts.  A
caller whose rules drift, or a new one that copies them and gets one wrong, fails here.  No kernel is launched."""
import importlib
import json
import os

import pytest

import spatial_desc_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_refusals.json")


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_tables_cover_what_they_should(recorded):
    nets, learners = recorded["refusals"]["net"], recorded["refusals"]["learner"]
    assert sorted(nets) == sorted(cases.NET_VIOLATIONS) and len(nets) == 32
    assert sorted(learners) == sorted(cases.LEARNERS)
    for rows in learners.values():
        assert sorted(rows) == sorted(list(cases.LEARNER_VIOLATIONS) + ["workspace_one_byte_short", "two_imposters"])
    assert sorted(recorded["accepts"]) == sorted(list(cases.modules(importlib.import_module("sus-net_amd"))) + ["reasons"])
    # every recorded refusal is one: SUSNET_E_INVALID and a message that starts with the entry point's name
    for row in nets.values():
        for call, (rc, msg) in row.items():
            assert rc == -1 and msg.startswith("susnet_spatial_forward: " if call == "forward" else "susnet_spatial_train_step: "), (call, msg)
    for entry, rows in learners.items():
        for name, (rc, msg) in rows.items():
            assert rc == -1 and msg.startswith(entry + ": "), (entry, name, msg)


def test_every_refusal_keeps_its_code_and_words(pkg, recorded):
    now = cases.record_refusals(pkg)
    for name, row in recorded["refusals"]["net"].items():
        for call, want in row.items():
            assert now["net"][name][call] == want, (name, call)
    for entry, rows in recorded["refusals"]["learner"].items():
        for name, want in rows.items():
            assert now["learner"][entry][name] == want, (entry, name)


def test_the_forward_and_the_learner_say_the_same_sentence(pkg):
    """The learner's message is the forward's once the struct prefixes and the entry point's name are taken off; the workspace query says
    what the step says."""
    for name, row in cases.record_refusals(pkg)["net"].items():
        sentence = row["forward"][1][len("susnet_spatial_forward: "):]
        for t in (0, 1):
            step = row[f"step_team{t}"][1]
            assert row[f"workspace_team{t}"] == row[f"step_team{t}"], name
            assert step[len("susnet_spatial_train_step: "):].replace(f"net[{t}].", "").replace(f"team[{t}].", "") == sentence, (name, t)


def test_the_two_learners_share_their_checks_words(pkg):
    rows = cases.record_refusals(pkg)["learner"]
    dense, spatial, dropout = (rows[e] for e in ("susnet_mlp_train_step", "susnet_spatial_train_step", "susnet_spatial_train_step_dropout"))
    for name in dense:
        strip = lambda entry, msg: msg[len(entry) + 2:]
        a, b, c = strip("susnet_mlp_train_step", dense[name][1]), strip("susnet_spatial_train_step", spatial[name][1]), \
            strip("susnet_spatial_train_step_dropout", dropout[name][1])
        if name.startswith("workspace"):  # (each names its own query and byte count)
            assert "susnet_mlp_train_workspace_bytes (" in a and "susnet_spatial_train_workspace_bytes (" in b and \
                "susnet_spatial_train_dropout_workspace_bytes (" in c, name
        else:
            assert a == b == c, name


def test_every_wrapper_keeps_its_accept_set(pkg, recorded):
    now = cases.record_accepts(pkg)
    for name, want in recorded["accepts"].items():
        for column, answer in want.items():
            assert now[name][column] == answer, (name, column)
    # the table has both answers in every column
    rows = [v for k, v in recorded["accepts"].items() if k != "reasons"]
    for column in ("qnet_is_none", "trainer", "trainer_dropout", "unserved_reason"):
        assert any(r[column] in (None, False) for r in rows) and any(r[column] not in (None, False) for r in rows), column
    assert recorded["accepts"]["dropout_two_layers"]["trainer"] is None and recorded["accepts"]["dropout_two_layers"]["trainer_dropout"]["p"] == 0.2


def test_the_description_is_what_the_wrappers_read(pkg):
    P = pkg.policy
    m = cases.modules(pkg)["fixture_notebook"]
    d = P.spatial_desc(m)
    assert (d["N"], d["C"], d["Fn"], d["k"], d["layers"], d["hidden"], d["p"]) == (9, 7, 15, 3, 3, 64, 0.0)
    assert d["convs"] == [(5, 1, 1, 1), (3, 1, 1, 1), (3, 1, 1, 1)] and d["sizes"] == [9, 9, 9, 9] and d["R"] == 3 * 81 + 15 and d["dims"] == [64, 16, 16, 5]
    net = P.SpatialQNet(cases.NoDevice(), m)
    assert (net.N, net.C, net.Fn, net.R, net.k, net.dims) == (d["N"], d["C"], d["Fn"], d["R"], d["k"], d["dims"])
    # fill_spatial_net writes the fields susnet_spatial_io and susnet_spatial_net share into either
    L = pkg._lib
    for dst in (L.SpatialIO(), L.SpatialNet()):
        P.fill_spatial_net(dst, d, 6)
        assert (dst.T, dst.N, dst.C, dst.Fn, dst.n_conv, dst.k, dst.rnn_layers, dst.rnn_hidden) == (6, 9, 7, 15, 3, 3, 3, 64)
        assert [(dst.conv_out[l], dst.conv_stride[l], dst.conv_padding[l], dst.conv_dilation[l]) for l in range(3)] == d["convs"]
    assert P.spatial_desc(pkg.policy.MLP([4, 3])) is None and P.spatial_desc(cases.modules(pkg)["hidden_256_two_layers"]) is None
