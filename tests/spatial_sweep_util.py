"""Shared by the tests of the SpatialDQN sweep step (susnet_spatial_train_sweep): K hand-made learners -- spatial_train_util.SpatialCall
objects, each with its own canaried buffers -- in ONE call, the dropout form of a single call for the twins, and bitwise comparison."""
import ctypes as C

import numpy as np
import torch

from train_exact import DEV, _workspace


def dropout_workspace(pkg, env, call):
    """Give ``call`` (a SpatialCall) the larger workspace the dropout step needs."""
    nbytes = C.c_uint64()
    pkg._lib.check(env.lib.susnet_spatial_train_dropout_workspace_bytes(env._h, C.byref(call.io), C.byref(nbytes)))
    call.nbytes = int(nbytes.value)
    call.ws = _workspace(call.nbytes)
    call.io.workspace, call.io.workspace_bytes = call.ws.data_ptr(), call.nbytes
    return call


def make_drop(pkg, p_online, p_target, seed, offset, row_base=0):
    """Two susnet_rnn_dropout ([imposter, crew]) with the same constants."""
    drop = (pkg._lib.RnnDropout * 2)()
    for t in range(2):
        drop[t].p[0], drop[t].p[1], drop[t].seed, drop[t].offset, drop[t].row_base = p_online, p_target, seed, offset, row_base
    return drop


def dropout_step(pkg, env, call, drop):
    """susnet_spatial_train_step_dropout on one SpatialCall: what a twin takes."""
    with torch.cuda.device(DEV):
        pkg._lib.check(env.lib.susnet_spatial_train_step_dropout(env._h, C.byref(call.io), drop, env._stream()))
    torch.cuda.synchronize()
    return call.results()


class SweepCall:
    """One susnet_spatial_train_sweep over ``calls`` (SpatialCall objects: the ios are copied when the object is built, so change a call's io
    before).  ``drops``: one pair of make_drop per call, or None.  The table has a canary behind it."""

    def __init__(self, pkg, env, calls, drops=None, envs=None):
        L = pkg._lib
        self.pkg, self.env, self.calls, K = pkg, env, list(calls), len(calls)
        self.ios = (L.SpatialTrainIO * K)(*[c.io for c in calls])
        self.envs = (C.c_void_p * K)(*[e._h for e in (envs or [env] * K)])
        nbytes = C.c_uint64()
        L.check(env.lib.susnet_spatial_train_sweep_table_bytes(K, C.byref(nbytes)))
        self.table_bytes = int(nbytes.value)
        self.table = _workspace(self.table_bytes)
        self.drops = None
        if drops is not None:
            self.drops = (L.RnnDropout * (2 * K))()
            for k, d in enumerate(drops):
                self.drops[2 * k], self.drops[2 * k + 1] = d[0], d[1]

    def call(self):
        """The raw return code (a refusal leaves susnet_last_error)."""
        return self.env.lib.susnet_spatial_train_sweep(self.envs, self.ios, self.drops, len(self.calls), self.table.data_ptr(), self.table_bytes,
                                                       self.env._stream())

    def launch(self):
        self.pkg._lib.check(self.call())

    def results(self):
        assert bool((self.table[self.table_bytes:] == 0x5A).all()), "the table was overrun"
        return [c.results() for c in self.calls]

    def step(self):
        with torch.cuda.device(DEV):
            self.launch()
        torch.cuda.synchronize()
        return self.results()


def same_bits(got, want, what=""):
    """(losses, per-team dicts) of SpatialCall.results(): every parameter, exp_avg, exp_avg_sq, step and the losses byte for byte."""
    assert np.array_equal(got[0].astype(np.float32).view(np.int32), want[0].astype(np.float32).view(np.int32)), f"{what} losses {got[0]} {want[0]}"
    for t in range(2):
        assert (got[1][t] is None) == (want[1][t] is None)
        if got[1][t] is None:
            continue
        for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "step"), got[1][t]["bits"], want[1][t]["bits"]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{what} team {t} {name}"
