"""The forward's launch census is pinned: which kernels a forward enqueues, how many of each, the workspace it asks for and -- with profiling on --
the launches, flops and bytes it books per profile family are EXACTLY what tests/golden/forward_census.json holds.

The fixture was written by tests/golden/make_forward_census.py on the commit before the forward's host code was split into named steps
(csrc/forward.hip), so a restructuring of that code that drops, adds or re-routes a launch fails here by name.  The cases are the smallest shapes
that reach each routing branch; each runs well under a second.  A deliberate change of the launch sequence regenerates the fixture with that script.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_forward_census", os.path.join(GOLD, "make_forward_census.py"))
mfc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfc)

with open(mfc.FIXTURE) as _f:
    FIXTURE = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(FIXTURE) == sorted(mfc.CASES)


@pytest.mark.parametrize("name", sorted(mfc.CASES))
def test_launch_census_matches_the_fixture(name):
    record, _ = mfc.run_case(name)  # (resets the process-wide debug switches in its `finally`)
    print(name, json.dumps(record))
    want = FIXTURE[name]
    assert [c["call"] for c in record["calls"]] == [c["call"] for c in want["calls"]]
    for got_c, want_c in zip(record["calls"], want["calls"]):
        assert got_c["kernels"] == want_c["kernels"], (name, got_c["call"])
        assert got_c["launches"] == want_c["launches"], (name, got_c["call"])
    assert record["workspace_bytes"] == want["workspace_bytes"]
    assert record.get("profile") == want.get("profile")  # {family: [launches, flops, bytes]}: exact, they are sums of integers below 2^53


def test_the_cases_reach_the_branches_they_are_named_for():
    """Read from the fixture itself, so that a regenerated fixture cannot quietly lose a branch."""
    k = {name: rec["calls"][-1]["kernels"] for name, rec in FIXTURE.items()}
    assert "ln1" not in k["tiny_ln_fold_1"] and "ln2" not in k["tiny_ln_fold_1"]            # LayerNorm folded into the 128-row GEMM's epilogues
    assert "norm1" not in k["tiny_no_self_attn"] and k["tiny_no_self_attn"]["norm3"] == 2
    assert k["tiny_attn_weights_head_1"]["attn_weights"] == 1
    assert k["vits_one_lane"]["panel"] == 2 and k["vits_default"]["panel"] == 4 and k["vits_panel4"]["panel4"] == 4
    assert "panel" not in k["vits_unfused"] and "rowln" not in k["vits_unfused"] and k["vits_unfused"]["norm3"] == 2
    assert k["vits_rowln_no_next"]["rowln"] == 6 and k["vits_rowln_no_next"]["gemm128"] > k["vits_default"]["gemm128"]
    assert k["vits_u8"]["patch_u8"] == 2 and "patch" not in k["vits_u8"]
    assert k["vitb_folded"]["ln_stats"] == 3 and k["vitb_folded"]["ln1"] == 1 and "ln2" not in k["vitb_folded"]
    assert "ln_stats" not in k["vitb_default"] and k["vitb_default"]["ln2"] == 4               # a fold256 handle's chunks of 228 rows
    assert "ln_stats" not in k["vitb_ln_fold_2"] and k["vitb_ln_fold_2"]["ln2"] == 2 and k["vitb_ln_fold_2"]["gemm256"] >= 9
    assert "ln_stats" not in k["vitb_gemm256_off"] and "gemm256" not in k["vitb_gemm256_off"]
    assert k["swiglu_default"]["silu_mul"] == 4 and k["swiglu_one_lane"]["silu_mul"] == 2
    assert FIXTURE["vits_profile"]["profile"]["40"][0] == 2 and FIXTURE["vits_profile"]["profile"]["42"][0] == 6
