"""Host-side checks of the fit scope table: head, tail, cross and layer are nested in their keys, each refuses another architecture
with its own exception, and the four backward workspaces have the sizes recorded in golden/fit_workspace_bytes.json (head, tail and cross from
the library as it was before the sizes were read from the carves the launches use, layer from the library as it was before the launches shared
their block steps: the layout must not move)."""
import dataclasses
import json
import os

import pytest

from crossscore_amd import _lib
from crossscore_amd.config import model_config
from crossscore_amd.model import FIT_CROSS, FIT_HEAD, FIT_LAYER, FIT_SCOPES, FIT_TAIL, CrossScoreNet, check_fit_supported

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = "synthetic/dinov2-tiny"
HAVE_LIBRARY = os.path.exists(_lib.LIB_PATH)  # (the checks of the library run where it is built, as in test_crossfit_host.py)
SCOPES = ("head", "tail", "cross", "layer")


def test_keys_are_nested():
    net = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY}))
    keys = {"head": net.HEAD_KEYS, "tail": net.TAIL_KEYS, "cross": net.CROSS_KEYS, "layer": net.LAYER_KEYS}
    assert [len(keys[s]) for s in SCOPES] == [4, 10, 16, 22]
    assert list(FIT_SCOPES) == list(SCOPES) and [s.name for s in FIT_LAYER.chain()] == ["layer", "cross", "tail", "head"]
    for scope in (FIT_TAIL, FIT_CROSS, FIT_LAYER):
        mine, parents = keys[scope.name], keys[scope.parent.name]
        assert mine[len(scope.own):] == parents and len(set(mine)) == len(mine)
    sd = net.state_dict()
    last = f"ref_cross.attn.layers.{net.arch.dec_layers - 1}."
    assert all(k in sd for k in keys["layer"]) and all(k.startswith(last) for k in keys["layer"][:18])
    assert FIT_HEAD.parent is None and FIT_HEAD.keep is None and FIT_TAIL.keep == "cs_fit_tail_keep" and FIT_CROSS.keep == "cs_fit_cross_keep"
    assert FIT_LAYER.keep == "cs_fit_layer_keep"
    for s in FIT_SCOPES.values():
        for name in (s.supported, s.backward, s.set_weights) + ((s.keep,) if s.keep else ()):
            assert name in _lib.SYMBOLS, name


def test_unsupported_architectures_are_refused_per_scope():
    if not HAVE_LIBRARY:
        return
    arch = CrossScoreNet(model_config(**{"backbone.from_pretrained": TINY})).arch
    assert arch.hidden == 128
    for scope in FIT_SCOPES:
        check_fit_supported(arch, scope)
    for scope, error, fragment in (("head", ValueError, "head fit"), ("tail", ValueError, "tail fit"), ("cross", NotImplementedError, "cross-attention fit"),
                                   ("layer", NotImplementedError, "whole-layer fit")):
        with pytest.raises(error, match=fragment):
            check_fit_supported(dataclasses.replace(arch, patch=16), scope)
    # without the decoder's self-attention the layer scope alone has nothing to fit
    plain = dataclasses.replace(arch, do_self_attn=False)
    for scope in ("head", "tail", "cross"):
        check_fit_supported(plain, scope)
    with pytest.raises(ValueError):
        check_fit_supported(plain, "layer")
    # a decoder head dim the attention backward is not built for (128 / 2 = 64) stops the cross and the layer scope, and those alone
    two = dataclasses.replace(arch, dec_heads=2)
    check_fit_supported(two, "head")
    check_fit_supported(two, FIT_TAIL)
    with pytest.raises(NotImplementedError, match="cross-attention fit"):
        check_fit_supported(two, "cross")
    with pytest.raises(NotImplementedError, match="whole-layer fit"):
        check_fit_supported(two, "layer")


def test_workspace_sizes_are_the_recorded_ones():
    if not HAVE_LIBRARY:
        return
    lib = _lib.load()
    rows = json.load(open(os.path.join(HERE, "golden", "fit_workspace_bytes.json")))
    assert len(rows) >= 12
    assert {r["B"] * r["Np"] for r in rows} == {1, 9, 63, 64, 65, 1369} and {r["C"] for r in rows} == {128, 384, 768}
    assert {r["N"] for r in rows} == {1, 5} and {r["C"] // r["heads"] for r in rows} == {16, 48, 96}
    for r in rows:
        M = r["B"] * r["Np"]
        got = {"head": lib.cs_head_backward_workspace_bytes(M, r["C"], 14), "tail": lib.cs_tail_backward_workspace_bytes(M, r["C"], 14),
               "cross": lib.cs_cross_backward_workspace_bytes(r["B"], r["Np"], r["N"], r["C"], 14, r["heads"]),
               "layer": lib.cs_layer_backward_workspace_bytes(r["B"], r["Np"], r["N"], r["C"], 14, r["heads"])}
        assert set(got) == set(SCOPES) and got == {k: r[k] for k in got}, r
        assert all(v % 256 == 0 for v in got.values()) and got["layer"] > got["cross"] > got["tail"] > got["head"] > 0, r
