"""Generator of tests/golden/g22_sdf_pack.json: what the host packers of the SDF network's weight streams (gens_amd.ops._pack_value_stream,
_pack_grad_stream, _pack_value_units, _pack_grad_pieces with two and three terms) and their slot tables (_value_slots, _value_pairs) emit
for 1 to 5 levels, as SHA-256 of the bytes + shape + dtype per tensor and the returned largest magnitudes as float.hex().  The streams are
the operands of five kernels: any change of a byte is a change of a layout.

    python tests/golden/make_golden_sdf_pack.py            # rewrites the file; on an unchanged packer the file does not change

The weights come from integer arithmetic, not from a random generator, so the digests do not depend on a library's generator: for layer k of
shape (o, i), with a = arange(o * i) and r = arange(o) in int64,
    w = ((((a * 2654435761 + 97 k + 12345) % 2^20).float() / 2^20) - 0.5) * (3 / sqrt(i)),   b = ((((r * 40503 + k) % 1024).float() / 1024) - 0.5) * 0.1
tests/test_sdf_pack_cpu.py recomputes every entry through `entries()` and compares it with the file."""
import hashlib
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PATH = os.path.join(HERE, "g22_sdf_pack.json")
LEVELS = (1, 2, 3, 4, 5)


def network(n_levels):
    k_in = 128 + 20 * n_levels
    dims = [(128, 27), (128, k_in), (101, k_in), (128, k_in), (128, k_in), (128, k_in), (1, k_in)]
    ws, bs = [], []
    for k, (o, i) in enumerate(dims):
        a = torch.arange(o * i, dtype=torch.int64)
        ws.append((((((a * 2654435761 + 97 * k + 12345) % 2 ** 20).float() / 2 ** 20) - 0.5) * (3.0 / math.sqrt(i))).reshape(o, i))
        r = torch.arange(o, dtype=torch.int64)
        bs.append(((((r * 40503 + k) % 1024).float() / 1024) - 0.5) * 0.1)
    return ws, bs


def digest(t):
    t = t.detach().cpu().contiguous()
    raw = t.view(torch.uint8) if t.numel() else t.new_empty(0, dtype=torch.uint8)
    return {"sha256": hashlib.sha256(raw.numpy().tobytes()).hexdigest(), "shape": list(t.shape), "dtype": str(t.dtype)}


def entries(n_levels):
    """{name: digest or float.hex()} of everything the packers return for one level count."""
    from gens_amd import ops
    ws, bs = network(n_levels)
    out = {}
    stream, w_out = ops._pack_value_stream(ws, bs, n_levels)
    out["value_stream"], out["value_stream.w_out"] = digest(stream), digest(w_out)
    stream, w_out = ops._pack_grad_stream(ws, bs, n_levels)
    out["grad_stream"], out["grad_stream.w_out"] = digest(stream), digest(w_out)
    units, w_out, vmax = ops._pack_value_units(ws, bs, n_levels)
    out["value_units"], out["value_units.w_out"], out["value_units.max"] = digest(units), digest(w_out), float(vmax).hex()
    for terms in (2, 3):
        pieces, vmax = ops._pack_grad_pieces(ws, bs, n_levels, terms=terms)
        out[f"grad_pieces{terms}"], out[f"grad_pieces{terms}.max"] = digest(pieces), float(vmax).hex()
    for name, tables in (("value_slots", ops._value_slots(n_levels)), ("value_pairs", ops._value_pairs(n_levels))):
        for part, t in zip(("hid", "pe", "cond"), tables):
            out[f"{name}.{part}"] = digest(t)
    return out


def main():
    doc = {str(n): entries(n) for n in LEVELS}
    with open(PATH, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in (3, 5):
        print(n, *(f"{k} {tuple(doc[str(n)][k]['shape'])} {doc[str(n)][k]['sha256'][:16]}"
                   for k in ("value_stream", "grad_stream", "value_units", "grad_pieces2", "grad_pieces3")), sep="\n   ")


if __name__ == "__main__":
    main()
