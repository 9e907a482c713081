"""hip_helpers.switches against a recording stand-in for the library (no GPU, no library): what it sets, what it puts back, and on which paths."""
import pytest

import hip_helpers as hh

DEFAULTS = {setter: default for setter, default in hh.SWITCHES.values()}


class _Recorder:
    """the five setters: every call is logged, `state` holds the value in force; the operand-type setter refuses what `refuse` holds"""

    def __init__(self, refuse=()):
        self.calls, self.state, self.refuse = [], dict(DEFAULTS), set(refuse)

    def __getattr__(self, name):
        if name not in DEFAULTS:
            raise AttributeError(name)

        def setter(v):
            self.calls.append((name, v))
            if name == "cs_debug_set_op_operand_dtype":
                if v in self.refuse:
                    return 3
                self.state[name] = v
                return 0
            self.state[name] = v

        return setter


def _defaults_are_the_library_s():
    assert DEFAULTS == {"cs_debug_set_op_operand_dtype": 0, "cs_debug_gemm256_enable": 1, "cs_debug_panel_impl": 0, "cs_debug_rowln_enable": 1,
                        "cs_debug_gemm_grid": 0}


GIVEN = [dict(bf16=True), dict(bf16=False, gemm256=False), dict(panel_impl=1, bf16=True), dict(rowln=2), dict(grid=8),
         dict(bf16=True, gemm256=False, panel_impl=1, rowln=0, grid=16), dict(bf16=None, grid=None)]


def _exit_resets_exactly_the_switches_that_were_set(given):
    lib = _Recorder()
    touched = {hh.SWITCHES[k][0] for k, v in given.items() if v is not None}
    with hh.switches(lib=lib, **given):
        assert {n for n, _ in lib.calls} == touched and len(lib.calls) == len(touched)
        for k, v in given.items():
            if v is not None:
                assert lib.state[hh.SWITCHES[k][0]] == int(v)
        inside = len(lib.calls)
    after = lib.calls[inside:]
    assert sorted(after) == sorted((n, DEFAULTS[n]) for n in touched)
    assert lib.state == DEFAULTS


def _exit_runs_when_the_body_raises():
    lib = _Recorder()
    with pytest.raises(ZeroDivisionError):
        with hh.switches(lib=lib, bf16=True, panel_impl=1):
            assert lib.state["cs_debug_panel_impl"] == 1
            1 / 0
    assert lib.state == DEFAULTS
    assert sorted(lib.calls[2:]) == [("cs_debug_panel_impl", 0), ("cs_debug_set_op_operand_dtype", 0)]


def _exit_runs_when_entry_fails_half_way():
    """the operand type is refused after the panel kernel was switched: the body never runs, both given switches go back, no other is touched"""
    lib = _Recorder(refuse={1})
    ran = []
    with pytest.raises(AssertionError):
        with hh.switches(lib=lib, panel_impl=1, bf16=True):
            ran.append(1)
    assert not ran and lib.state == DEFAULTS
    assert lib.calls[:2] == [("cs_debug_panel_impl", 1), ("cs_debug_set_op_operand_dtype", 1)]
    assert sorted(lib.calls[2:]) == [("cs_debug_panel_impl", 0), ("cs_debug_set_op_operand_dtype", 0)]


def _nested_managers_over_different_switches():
    lib = _Recorder()
    with hh.switches(lib=lib, bf16=True, gemm256=False):
        with hh.switches(lib=lib, grid=8):
            assert lib.state == {**DEFAULTS, "cs_debug_set_op_operand_dtype": 1, "cs_debug_gemm256_enable": 0, "cs_debug_gemm_grid": 8}
        assert lib.state == {**DEFAULTS, "cs_debug_set_op_operand_dtype": 1, "cs_debug_gemm256_enable": 0}  # the outer setting is still in force
        assert lib.calls[-1] == ("cs_debug_gemm_grid", 0)
    assert lib.state == DEFAULTS


def _an_unknown_switch_is_refused_before_anything_is_set():
    lib = _Recorder()
    with pytest.raises(AssertionError):
        with hh.switches(lib=lib, bf16=True, gemm512=True):
            pass
    assert lib.calls == []


def test_switch_manager_against_a_recording_library():
    _defaults_are_the_library_s()
    for given in GIVEN:
        _exit_resets_exactly_the_switches_that_were_set(given)
    _exit_runs_when_the_body_raises()
    _exit_runs_when_entry_fails_half_way()
    _nested_managers_over_different_switches()
    _an_unknown_switch_is_refused_before_anything_is_set()
