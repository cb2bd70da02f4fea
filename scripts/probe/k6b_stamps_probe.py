#!/usr/bin/env python3
"""Where the waves of K6b's gradient kernel (sdf_bf16x3_k<3, true>) spend their cycles: s_memtime stamps around every chunk boundary of the
weight ring (its vmcnt wait, its barrier, its refill issues) and around every layer's activation / split phase, summed per wave of the
workgroup over one chunk of 32 768 rays x 128 samples at three levels and the bench's volume sizes.
Build:  make -C gens_amd/csrc stamps      Run:  GENS_HIP_LIB=gens_amd/csrc/stamps/libgens_hip_k6b_stamps.so python scripts/probe/k6b_stamps_probe.py
Stamps cost cycles of their own: read the SHARES, not the totals (the cost of one stamp is measured in the kernel and taken off)."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from gens_amd import lib as L, ops, synthetic  # noqa: E402
from gens_amd.config import gens_model_conf  # noqa: E402
from gens_amd.models.modules.sdf_network import SDFNetwork  # noqa: E402

RAYS, SAMPLES, DIMS = 32768, 128, (256, 128, 64)
KINDS = ["products: MFMAs, their LDS reads, what sits in their gaps", "boundary: vmcnt wait", "boundary: barrier", "boundary: refill issues",
         "forward: softplus and split", "reverse: softplus' product and split", "chain rule to x"]

torch.manual_seed(0)
net = SDFNetwork(**gens_model_conf(volume_dims=DIMS)["implicit_surface"]["sdf_network"])
with torch.no_grad():
    for p in net.parameters():
        p.add_(0.02 * torch.randn_like(p))
net = net.cuda()
packed = ops.VolumeSet.packed([v.cuda() for v in synthetic.make_volumes(list(DIMS), seed=3)])
plan = ops.SdfMlpPlan(net)
g = torch.Generator().manual_seed(1)
o = torch.rand(RAYS, 1, 3, generator=g) * 1.6 - 0.8               # rays through the cube, samples in order along each ray like render_core's
d = torch.nn.functional.normalize(torch.randn(RAYS, 1, 3, generator=g), dim=-1)
t = torch.linspace(-0.6, 0.6, SAMPLES).view(1, SAMPLES, 1)
pts = (o + t * d).reshape(-1, 3).cuda()

fn = L.load().gens_debug_k6b_stamps
buf = (ctypes.c_ulonglong * (4 * 16))()
for rep in range(3):                                              # the last launch is the one read
    assert fn(buf, 1) == 0
    ops.sdf_mlp(plan, packed, pts, want_grad=True)
    torch.cuda.synchronize()
assert fn(buf, 0) == 0
print(f"sdf_bf16x3_k<3, true>, {RAYS} x {SAMPLES} points, volumes {DIMS}: cycles per wave (mean over workgroups), one stamp's own cost taken off")
for w in range(4):
    v = [buf[w * 16 + i] for i in range(16)]
    wgs = v[15]
    if not wgs:
        print(f"wave {w}: no stamps")
        continue
    cost = v[7] / wgs
    net_c = [max(v[k] / wgs - cost * v[8 + k] / wgs, 0.0) for k in range(7)]
    total = sum(net_c)
    print(f"wave {w}: {wgs} workgroups, one stamp {cost:.0f} cycles, {sum(v[8:15]) // wgs} stamps, {sum(v[:7]) / wgs:.0f} cycles stamped, {total:.0f} without the stamps")
    for k in range(7):
        n = v[8 + k] / wgs
        print(f"   {KINDS[k]:58s} {net_c[k]:9.0f}  {100 * net_c[k] / total:5.1f} %   {n:5.0f} x {net_c[k] / n if n else 0:7.1f}")
