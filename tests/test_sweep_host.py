"""The host side of the sweep (run_sweep's variants and directories, the chunking of DeviceDQNSweepTrainer, the C ABI entry): no GPU."""
import ctypes as C
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("sus-net_amd")


def test_variant_validation(pkg):
    tl = pkg.train_loop
    assert set(tl.SWEEP_VARIANT_KEYS) == {"gamma", "learning_rate", "seed", "scheduler_start_eps", "scheduler_end_eps", "scheduler_time_steps", "name"}
    full = {"gamma": 0.9, "learning_rate": 1e-3, "seed": 3, "scheduler_start_eps": 1.0, "scheduler_end_eps": 0.1, "scheduler_time_steps": 10, "name": "a"}
    out = tl.check_variants([full, {}, {"gamma": 0.8}])
    assert out == [full, {}, {"gamma": 0.8}] and out[0] is not full
    for bad in ("batch_size", "num_steps", "train_step_interval", "components", "Gamma"):
        with pytest.raises(ValueError, match=bad):
            tl.check_variants([{"gamma": 0.9}, {bad: 1}])
    with pytest.raises(ValueError, match="variant 1"):
        tl.check_variants([{"gamma": 0.9}, {"batch_size": 1}])
    with pytest.raises(ValueError, match="no variants"):
        tl.check_variants([])
    # refused before anything is built: the factories are never called
    boom = lambda *a: (_ for _ in ()).throw(AssertionError("built"))
    with pytest.raises(ValueError, match="batch_size"):
        pkg.run_sweep(boom, [{"batch_size": 4}], 10, boom, boom, ["onehot_pos"])
    with pytest.raises(ValueError, match="no variants"):
        pkg.run_sweep(boom, [], 10, boom, boom, ["onehot_pos"])
    with pytest.raises(ValueError, match="sequence_length"):
        pkg.run_sweep(boom, [{}], 10, boom, boom, ["onehot_pos"], sequence_length=2)


def test_member_directories(pkg, tmp_path):
    tl = pkg.train_loop
    dirs = tl.sweep_member_dirs(tmp_path, [{"gamma": 0.99}, {"name": "g0.9"}, {"gamma": 0.8, "name": 7}], "2024-01-02_03-04-05")
    assert dirs == [tmp_path / "0" / "2024-01-02_03-04-05", tmp_path / "g0.9" / "2024-01-02_03-04-05", tmp_path / "7" / "2024-01-02_03-04-05"]
    with pytest.raises(ValueError, match="repeat"):
        tl.sweep_member_dirs(tmp_path, [{"name": "1"}, {}], "t")


def test_chunks_of_at_most_sixteen_in_order(pkg):
    L, tr = pkg._lib, pkg.trainer
    assert L.DQN_MAX_LEARNERS == 16
    assert tr.sweep_chunks(35) == [(0, 16), (16, 32), (32, 35)]
    assert tr.sweep_chunks(16) == [(0, 16)] and tr.sweep_chunks(17) == [(0, 16), (16, 17)] and tr.sweep_chunks(1) == [(0, 1)]
    assert tr.sweep_chunks(0) == []
    for k in range(1, 70):
        chunks = tr.sweep_chunks(k)
        assert [i for lo, hi in chunks for i in range(lo, hi)] == list(range(k)) and all(0 < hi - lo <= 16 for lo, hi in chunks)
    with pytest.raises(ValueError, match="at least one"):
        pkg.DeviceDQNSweepTrainer([])


def test_the_entry_point_is_declared_exported_and_prototyped(pkg):
    L = pkg._lib
    header = open(os.path.join(ROOT, "include", "susnet.h")).read()
    assert re.search(r"#define\s+SUSNET_DQN_MAX_LEARNERS\s+16\b", header)
    m = re.search(r"int\s+susnet_dqn_train_sweep\(([^)]*)\);", header)
    assert m, "susnet_dqn_train_sweep is not declared"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["susnet_env *const *envs", "const susnet_dqn_io *ios", "int32_t n_learners", "void *stream"]
    assert "susnet_dqn_train_sweep" in L.EXPORTS and re.fullmatch(r"susnet_[a-z_]+", "susnet_dqn_train_sweep")
    assert re.search(r"#define\s+SUSNET_ABI_VERSION\s+%d\b" % L.ABI_VERSION, header)  # (the entry point is an addition: no struct or existing call changes)
    fn = L.lib().susnet_dqn_train_sweep
    assert fn.argtypes == [C.POINTER(C.c_void_p), C.POINTER(L.DqnIO), C.c_int32, C.c_void_p] and fn.restype == C.c_int
    # refused on the host, before any device call: null tables and learner counts outside 1 .. 16
    ios, envs = (L.DqnIO * 1)(), (C.c_void_p * 1)()
    assert fn(None, ios, 1, None) == L.E_INVALID
    for n in (0, -1, 17):
        assert fn(envs, ios, n, None) == L.E_INVALID and b"n_learners" in L.lib().susnet_last_error()
    assert fn(envs, ios, 1, None) == L.E_INVALID and b"learner 0" in L.lib().susnet_last_error()  # (a null handle)
