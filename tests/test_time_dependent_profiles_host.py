"""Host logic of time-dependent wall velocities (no device): the reference's arity rule for profile(cells, timestep)
(bc_hybrid.py:163-172), the chunk plan of a run, the pairing condition of reference-style calls, and what a run stages before each
launch (a recording fake of the native stepper)."""

import functools

import numpy as np
import pytest

import xlb_amd
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC, HybridBC
from xlb_amd.operator.boundary_condition.boundary_condition import profile_is_time_dependent
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper
from xlb_amd.operator.stepper.nse_stepper import chunk_plan, pairs_in_time


def _one(cells):
    return cells


def _two(cells, timestep):
    return cells


def _scaled(scale, cells, timestep):
    return scale * cells


class _Spin:
    def __call__(self, cells, timestep):
        return cells


class _Still:
    def __call__(self, cells):
        return cells


class _Opaque:
    """a callable whose signature cannot be inspected"""

    @property
    def __signature__(self):
        raise ValueError("no signature")

    def __call__(self, *args):
        return args[0]


def test_arity_rule():
    assert not profile_is_time_dependent(_one)
    assert profile_is_time_dependent(_two)
    assert profile_is_time_dependent(lambda cells, t: cells)
    assert not profile_is_time_dependent(lambda cells: cells)
    assert profile_is_time_dependent(lambda cells, t=0: cells)  # (parameters are counted, defaults included)
    assert profile_is_time_dependent(functools.partial(_scaled, 2.0))
    assert profile_is_time_dependent(functools.partial(_scaled, 2.0, timestep=3))  # (a keyword-bound parameter is still listed)
    assert not profile_is_time_dependent(functools.partial(_two, np.zeros(1)))  # (positionally bound: one parameter left)
    assert profile_is_time_dependent(_Spin())
    assert not profile_is_time_dependent(_Still())
    assert not profile_is_time_dependent(_Opaque())


def test_is_time_dependent_attribute_and_shape_error_name_t():
    pp = xlb_amd.PrecisionPolicy.FP32FP32
    vs = xlb_amd.velocity_set.D3Q19(pp, xlb_amd.ComputeBackend.HIP)
    kw = dict(velocity_set=vs, precision_policy=pp, compute_backend=xlb_amd.ComputeBackend.HIP, indices=[[1], [1], [1]])
    assert HalfwayBounceBackBC(profile=lambda c, t: c, **kw).is_time_dependent
    assert not HalfwayBounceBackBC(profile=lambda c: c, **kw).is_time_dependent
    assert not HalfwayBounceBackBC(prescribed_value=(0.0, 0.0, 0.0), **kw).is_time_dependent
    assert HybridBC("bounceback_grads", profile=_Spin(), **kw).is_time_dependent
    assert not HybridBC("bounceback_grads", profile=_Still(), **kw).is_time_dependent

    def late(cells, t):
        v = np.full((3, cells.shape[1]), 0.01 * t)
        return v if t < 3 else v[:2]

    bc = HalfwayBounceBackBC(profile=late, **kw)
    cells = np.array([[1, 2], [3, 4], [5, 6]])
    bc._evaluate_profile(cells, np.array([7, 9]))  # t = 0: shapes agree
    assert bc._profile_table(None) is None and list(bc._td_keys) == [7, 9]
    v = bc.profile_at(2)
    assert v.shape == (2, 3) and np.array_equal(v, np.full((2, 3), np.float32(0.02)).astype(np.float64))
    with pytest.raises(ValueError, match=r"t=3"):
        bc.profile_at(3)
    bad0 = HalfwayBounceBackBC(profile=lambda c, t: np.zeros((2, 1)), **kw)
    with pytest.raises(ValueError, match=r"t=0"):
        bad0._evaluate_profile(cells, np.array([7, 9]))  # (prepare_fields fails early)


def test_chunk_plan():
    assert chunk_plan(0, 8) == []
    assert chunk_plan(1, 64) == [1]
    assert chunk_plan(7, 64) == [7]
    assert chunk_plan(70, 64) == [32, 32, 6]
    assert chunk_plan(5, 4) == [2, 2, 1]
    assert chunk_plan(13, 10) == [4, 4, 4, 1]  # (half of 10 is 5: rounded down to an even size)
    for n in range(0, 60):
        for slots in (4, 6, 10, 64):
            plan = chunk_plan(n, slots)
            assert sum(plan) == n and all(0 < k <= slots // 2 for k in plan)
            assert all(k % 2 == 0 for k in plan[:-1])


def test_pairing_condition():
    assert pairs_in_time(4, 5, True)
    assert not pairs_in_time(4, 4, True) and not pairs_in_time(4, 6, True) and not pairs_in_time(4, 3, True)
    assert pairs_in_time(4, 4, False) and pairs_in_time(4, 9, False)  # (without time-dependent walls the timestep does not matter)


class _FakeNative:
    """records what the stepper stages and launches; `run` answers like xlbhip_run_any (result in f_b after an odd count)"""

    def __init__(self, slots):
        self.slots = slots
        self.log = []
        self.resident = {}

    def stage_bc_profiles(self, t_first, values):
        assert values.shape[0] <= self.slots
        for k in range(values.shape[0]):
            self.resident[t_first + k] = values[k].copy()
        self.log.append(("stage", t_first, values.shape[0]))

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        for t in range(first_timestep, first_timestep + n_steps):
            assert t in self.resident and np.all(self.resident[t] == t), t  # staged before the launch, with t's values
        self.log.append(("run", first_timestep, n_steps))
        return n_steps % 2 == 1


class _FakeBC:
    def __init__(self, n):
        self._td_keys = np.arange(n, dtype=np.uint32)

    def profile_at(self, t, out=None):
        v = np.full((self._td_keys.size, 3), float(t))
        if out is not None:
            out[...] = v
        return v


def _fake_stepper(slots):
    s = object.__new__(IncompressibleNavierStokesStepper)
    s._native = _FakeNative(slots)
    s._td_bcs = [_FakeBC(3), _FakeBC(2)]
    s._td_slots = slots
    return s


def test_chunked_run_stages_every_chunk_before_its_launch():
    s = _fake_stepper(8)
    fa, fb = object(), object()
    cur, oth = s._run_chunked(fa, fb, None, None, 1.0, 13, 5)
    assert s._native.log == [("stage", 5, 4), ("run", 5, 4), ("stage", 9, 4), ("run", 9, 4), ("stage", 13, 4), ("run", 13, 4),
                             ("stage", 17, 1), ("run", 17, 1)]
    assert (cur, oth) == (fb, fa)  # three even chunks, then one single step
    rows = s._td_rows(3, 2)
    assert rows.shape == (2, 5, 3) and np.all(rows[0] == 3) and np.all(rows[1] == 4)
    assert s._run_chunked(fa, fb, None, None, 1.0, 0, 5) == (fa, fb)


def test_a_profile_failing_in_a_later_chunk_says_where_the_run_stands():
    class _Bad(_FakeBC):
        def profile_at(self, t, out=None):
            if t >= 9:
                raise ValueError(f"wrong shape at t={t}")
            return super().profile_at(t, out)

    s = _fake_stepper(8)
    s._td_bcs = [_Bad(3)]
    fa, fb = object(), object()
    with pytest.raises(ValueError, match=r"t=9 \(the run stopped at timestep 9: f\(9\) is in the field passed as f_0\)") as ei:
        s._run_chunked(fa, fb, None, None, 1.0, 13, 5)
    assert ei.value.timestep_reached == 9 and ei.value.fields == (fa, fb)
    assert s._native.log == [("stage", 5, 4), ("run", 5, 4)]  # (the first chunk ran; nothing after it)
    s = _fake_stepper(8)
    s._td_bcs = [_Bad(3)]
    with pytest.raises(ValueError, match=r"^wrong shape at t=9$"):
        s._run_chunked(fa, fb, None, None, 1.0, 5, 6)  # a failure in the first chunk (6 .. 9): nothing was enqueued
    assert s._native.log == []
