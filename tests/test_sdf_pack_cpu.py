"""The host side of the fused SDF network without a GPU.

Packers (gens_amd/ops/sdf_pack.py): every stream, output row, largest magnitude and slot table for 1 to 5 levels must be bit for bit what
tests/golden/g22_sdf_pack.json records (SHA-256 + shape + dtype; weights from integer arithmetic, tests/golden/make_golden_sdf_pack.py).  The
streams are the operands of five kernels, so a changed digest is a changed layout.  What the streams MEAN is checked by the lane-for-lane
emulations of test_value_units_cpu.py and test_grad_pieces.py.

Routing (gens_amd.ops._sdf_route): which entry point a launch of sdf_mlp takes, on stub plans."""
import json
import os
import sys
import types

import pytest

from gens_amd import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_sdf_pack as G  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(G.PATH) as f:
        return json.load(f)


def test_golden_covers_every_level_count(recorded):
    assert sorted(recorded) == [str(n) for n in G.LEVELS] == ["1", "2", "3", "4", "5"]


@pytest.mark.parametrize("n_levels", G.LEVELS)
def test_streams_bit_identical(recorded, n_levels):
    want, got = recorded[str(n_levels)], G.entries(n_levels)
    assert sorted(got) == sorted(want)
    assert len(got) == 17              # 5 streams, 3 output rows, 3 largest magnitudes, 2 x 3 tables
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_generator_matches_the_published_digests(recorded):
    """Cross-check of the weight recipe: leading digits computed independently of this generator, on the packers as they stood before they were
    folded onto sdf_pack.py's shared pieces."""
    lead = {"3": {"value_stream": ([126, 4, 64, 4], "238091f3ec2a2f2f"), "grad_stream": ([251, 4, 64, 4], "d4ed028d96d89f7d"),
                  "value_units": ([64, 4, 2, 64, 8], "ad2a13509fa3398e"), "grad_pieces2": ([1016, 64, 8], "4268192072cc62f8"),
                  "grad_pieces3": ([1520, 64, 8], "9570778805006de1")},
            "5": {"value_stream": ([151, 4, 64, 4], "ae7195dbc1b31a6c"), "grad_stream": ([315, 4, 64, 4], "c4853a323cfb85ee"),
                  "value_units": ([80, 4, 2, 64, 8], "f319eb78cf303b7e"), "grad_pieces2": ([1288, 64, 8], "04382f1537cab7d4"),
                  "grad_pieces3": ([1936, 64, 8], "7853360032ea66dc")}}
    for n, rows in lead.items():
        for name, (shape, head) in rows.items():
            assert recorded[n][name]["shape"] == shape and recorded[n][name]["sha256"].startswith(head), (n, name)


def test_tables_are_one_function_of_the_width():
    import torch
    for n in G.LEVELS:
        for width, tables in ((8, ops._value_slots(n)), (4, ops._value_pairs(n))):
            for a, b in zip(tables, ops._slot_tables(n, width)):
                assert torch.equal(a, b) and a.shape[1:] == (2, width)


# ------------------------------------------------------------------------------------------------------------------------------------
# routing
# ------------------------------------------------------------------------------------------------------------------------------------
def _plan(grad_pieces=object(), bf16x3_pieces=object(), value_ok=True):
    return types.SimpleNamespace(grad_pieces=grad_pieces, bf16x3_pieces=bf16x3_pieces, value_ok=value_ok)


def _kernels(sdf_value="bf16x3", sdf_grad="bf16x3", sdf_grad_f16=True):
    return types.SimpleNamespace(sdf_value=sdf_value, sdf_grad=sdf_grad, sdf_grad_f16=sdf_grad_f16)


def _routes(plan, precision, kernels):
    """(value entry, gradient entry); every route but gens_sdf_mlp is its own profile label."""
    out = []
    for want_grad in (False, True):
        entry, label = ops._sdf_route(plan, want_grad, precision, kernels)
        assert label == entry or entry == "gens_sdf_mlp"
        out.append(entry)
    return tuple(out)


def test_route_defaults():
    assert _routes(_plan(), "f32", _kernels()) == ("gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3")
    assert _routes(_plan(), "f32", ops.KernelChoice(env={})) == ("gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3")


def test_route_without_bf16x3_pieces():
    assert _routes(_plan(bf16x3_pieces=None), "f32", _kernels()) == ("gens_sdf_value", "gens_sdf_grad")


def test_route_transposed():
    assert _routes(_plan(), "f32", _kernels("transposed", "transposed")) == ("gens_sdf_value", "gens_sdf_grad")
    assert _routes(_plan(bf16x3_pieces=None), "f32", _kernels("transposed", "transposed")) == ("gens_sdf_value", "gens_sdf_grad")


def test_route_rowmajor_and_its_labels():
    assert _routes(_plan(), "f32", _kernels("rowmajor", "rowmajor")) == ("gens_sdf_mlp", "gens_sdf_mlp")
    assert ops._sdf_route(_plan(), False, "f32", _kernels("rowmajor", "rowmajor")) == ("gens_sdf_mlp", "gens_sdf_mlp:value")
    assert ops._sdf_route(_plan(), True, "f32", _kernels("rowmajor", "rowmajor")) == ("gens_sdf_mlp", "gens_sdf_mlp:grad")
    # one generation per pass: the two switches are independent
    assert _routes(_plan(), "f32", _kernels("rowmajor", "bf16x3")) == ("gens_sdf_mlp", "gens_sdf_grad_bf16x3")
    assert _routes(_plan(), "f32", _kernels("transposed", "rowmajor")) == ("gens_sdf_value", "gens_sdf_mlp")


def test_route_split_half():
    assert _routes(_plan(), "f16x2", _kernels()) == ("gens_sdf_value_f16", "gens_sdf_grad_f16")
    assert _routes(_plan(), "f16x2", _kernels("rowmajor", "rowmajor")) == ("gens_sdf_value_f16", "gens_sdf_grad_f16")
    assert _routes(_plan(), "f16x2", _kernels("transposed", "transposed")) == ("gens_sdf_value_f16", "gens_sdf_grad_f16")


def test_route_split_half_gradient_switched_off():
    assert _routes(_plan(), "f16x2", _kernels(sdf_grad_f16=False)) == ("gens_sdf_value_f16", "gens_sdf_grad_bf16x3")
    assert _routes(_plan(), "f16x2", _kernels("transposed", "transposed", sdf_grad_f16=False)) == ("gens_sdf_value_f16", "gens_sdf_grad")


def test_route_split_half_out_of_range():
    assert _routes(_plan(grad_pieces=None, value_ok=False), "f16x2", _kernels()) == ("gens_sdf_value_bf16x3", "gens_sdf_grad_bf16x3")
    assert _routes(_plan(grad_pieces=None, value_ok=False, bf16x3_pieces=None), "f16x2", _kernels()) == ("gens_sdf_value", "gens_sdf_grad")
    assert _routes(_plan(grad_pieces=None, value_ok=False), "f16x2", _kernels("rowmajor", "rowmajor")) == ("gens_sdf_mlp", "gens_sdf_mlp")


def test_every_stream_route_has_its_launch_data():
    """_SDF_STREAMS names plan attributes that SdfMlpPlan.__init__ sets, and covers exactly the six stream kernels."""
    import inspect
    assert sorted(ops._SDF_STREAMS) == sorted(f"gens_sdf_{k}{s}" for k in ("value", "grad") for s in ("", "_f16", "_bf16x3"))
    src = inspect.getsource(ops.SdfMlpPlan.__init__)
    for entry, (stream, _, row, scaled, stash, _) in ops._SDF_STREAMS.items():
        assert f"self.{stream}" in src and f"self.{row}" in src
        assert (stash is not None) == entry.startswith("gens_sdf_grad")
        assert scaled == (entry == "gens_sdf_grad_f16")
