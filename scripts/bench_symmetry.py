#!/usr/bin/env python3
"""The per-row board symmetries (gvec_obs_symmetry, obs_symmetry_kernel) on a replay batch - s and ns (nine planes each), the
legal mask of 5 H W bytes and the action - against the same definition written in torch, in one process:
  hip     one launch.  `launch` times the C entry point on preallocated outputs (device events around --calls launches);
          `front` times symmetry.apply_symmetry, which allocates its outputs (wall clock, one synchronisation per repeat)
  torch   the half-move rule and the source tile of every destination tile computed per row on the device, an int64 gather
          index [rows, 9, H W] for the planes (used for s and for ns) and a second one [rows, 5 H W] for the mask, then three
          gathers, and the action by its own arithmetic.  The indices depend on the batch's sym, so building them is part of
          every call.
The two results are compared bit for bit before anything is timed.  Each shape runs twice: sym uniform over the eight
symmetries with uniformly random actions (a fifth of them half moves, most of which fall back to the identity), and every
row transposed (sym 4, full moves only so that no row falls back): the kernel's worst read pattern, stride W.
Bytes by construction: every byte of every tensor is read once and written once, rows * (2 * (2 * 9 * H W * 4 + 5 H W + 8) + 2);
the floor is that over the copy rate bench.py reports (--copy-tbs).
usage: scripts/bench_symmetry.py [--calls K] [--repeats R] [--skip-torch] [--configs rows:WxH,...] [--out file.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--configs", default="16384:20x20,1024:15x15", help="rows:WxH")
ap.add_argument("--copy-tbs", type=float, default=6.29)
ap.add_argument("--skip-torch", action="store_true", help="time the launch alone (sweeps over row counts)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import ctypes as C  # noqa: E402

import torch  # noqa: E402

from generalsreinforcementlearning_amd import _lib as lib  # noqa: E402
from generalsreinforcementlearning_amd.symmetry import apply_symmetry  # noqa: E402

DEV = torch.device("cuda", 0)
TABLES = torch.tensor([[0, 1, 2, 3, 4], [0, 3, 2, 1, 4], [2, 1, 0, 3, 4], [2, 3, 0, 1, 4], [3, 2, 1, 0, 4], [3, 0, 1, 2, 4], [1, 2, 3, 0, 4],
                       [1, 0, 3, 2, 4]], device=DEV)
INVERSE = torch.tensor([0, 1, 2, 3, 4, 6, 5, 7], device=DEV)


def wall(fn, calls, repeats):
    """median over the repeats of the wall time per call: every call enqueued, one synchronisation per repeat"""
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / calls)
    runs.sort()
    return runs[len(runs) // 2], runs[0], runs[-1]


def device_time(fn, calls, repeats):
    """median over the repeats of the device time per call, from events around `calls` calls"""
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) * 1e-3 / calls)
    runs.sort()
    return runs[len(runs) // 2], runs[0], runs[-1]


def half_dir(x, y, W, H):
    return torch.where(y > 0, 0, torch.where(x < W - 1, 1, torch.where(y < H - 1, 2, 3)))


def image(sym, x, y, W, H):
    x = torch.where((sym & 1) != 0, W - 1 - x, x)
    y = torch.where((sym & 2) != 0, H - 1 - y, y)
    tr = (sym & 4) != 0
    return torch.where(tr, y, x), torch.where(tr, x, y)


def torch_symmetry(sym, s, ns, mask, action, W, H):
    rows, HW = sym.shape[0], W * H
    sym = sym.long()
    # the half-move rule
    at, ad = action // 5, action % 5
    ax, ay = at % W, at // W
    gx, gy = image(sym, ax, ay, W, H)
    exact = half_dir(gx, gy, W, H) == TABLES[sym, half_dir(ax, ay, W, H)]
    sym = torch.where((ad == 4) & ~exact, 0, sym)
    # the action
    gx, gy = image(sym, ax, ay, W, H)
    action2 = 5 * (gy * W + gx) + TABLES[sym, ad]
    # the source tile of every destination tile: the steps of g undone in reverse order
    t = torch.arange(HW, device=DEV)
    ty, tx = (t // W)[None, :], (t % W)[None, :]
    tr = ((sym & 4) != 0)[:, None]
    x, y = torch.where(tr, ty, tx), torch.where(tr, tx, ty)
    x = torch.where(((sym & 1) != 0)[:, None], W - 1 - x, x)
    y = torch.where(((sym & 2) != 0)[:, None], H - 1 - y, y)
    src = y * W + x                                                            # int64 [rows, HW]
    idx = src[:, None, :].expand(rows, 9, HW)
    s2 = s.reshape(rows, 9, HW).gather(2, idx).reshape(s.shape)
    ns2 = ns.reshape(rows, 9, HW).gather(2, idx).reshape(ns.shape)
    midx = (5 * src[:, :, None] + TABLES[INVERSE[sym]][:, None, :]).reshape(rows, 5 * HW)
    return s2, ns2, mask.gather(1, midx), action2, sym.to(torch.uint8)


res = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "repeats": args.repeats, "copy_tbs": args.copy_tbs, "shapes": []}
gen = torch.Generator(device=DEV)
gen.manual_seed(1)
L = lib.load()
for c in args.configs.split(","):
    r, wh = c.split(":")
    W, H = (int(v) for v in wh.split("x"))
    rows, HW, A = int(r), W * H, 5 * W * H
    s, ns = (torch.rand(rows, 9, H, W, device=DEV, generator=gen) for _ in range(2))
    mask = torch.rand(rows, A, device=DEV, generator=gen) < 0.3
    for pattern in ("uniform", "transpose"):
        if pattern == "uniform":
            sym = torch.randint(0, 8, (rows,), dtype=torch.uint8, device=DEV, generator=gen)
            action = torch.randint(0, A, (rows,), device=DEV, generator=gen)
        else:
            sym = torch.full((rows,), 4, dtype=torch.uint8, device=DEV)
            action = 5 * torch.randint(0, HW, (rows,), device=DEV, generator=gen) + torch.randint(0, 4, (rows,), device=DEV, generator=gen)
        row = {"config": c, "sym": pattern, "rows": rows, "bytes_per_row": 2 * (2 * 9 * HW * 4 + A + 8) + 2}
        row["bytes"] = rows * row["bytes_per_row"]
        row["floor_us"] = row["bytes"] / (args.copy_tbs * 1e12) * 1e6
        got = apply_symmetry(sym, (s, ns), mask=mask, action=action, return_applied=True)
        want = got if args.skip_torch else torch_symmetry(sym, s, ns, mask, action, W, H)
        row["equal_to_torch"] = None if args.skip_torch else all(bool(torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32)
                                                     if w.dtype == torch.float32 else w)) for g, w in zip(got, want))
        row["rows_fallen_back"] = int((got[4] != sym).sum())
        # the C entry point on preallocated outputs
        outs = [torch.empty_like(x) for x in got]
        a = lib.ObsSymmetryArgs(rows=rows, width=W, height=H, num_sets=2, inverse=0, reserved=0, sym=sym.data_ptr(),
                                mask_in=mask.data_ptr(), mask_out=outs[2].data_ptr(), action_in=action.data_ptr(),
                                action_out=outs[3].data_ptr(), applied=outs[4].data_ptr())
        for k, x in enumerate((s, ns)):
            a.sets[k].in_, a.sets[k].out, a.sets[k].planes, a.sets[k].in_row_stride = x.data_ptr(), outs[k].data_ptr(), 9, 9 * HW
        stream = torch.cuda.current_stream(DEV).cuda_stream

        def launch():
            lib.check(L.gvec_obs_symmetry(0, stream, C.byref(a)), "gvec_obs_symmetry")

        launch()
        row["launch_equal_to_front"] = all(bool(torch.equal(o.view(torch.uint8), g.view(torch.uint8))) for o, g in zip(outs, got))
        for name, fn, timer in (("launch_device", launch, device_time), ("launch_wall", launch, wall),
                                ("front_wall", lambda: apply_symmetry(sym, (s, ns), mask=mask, action=action, return_applied=True), wall),
                                ("torch_device", lambda: torch_symmetry(sym, s, ns, mask, action, W, H), device_time),
                                ("torch_wall", lambda: torch_symmetry(sym, s, ns, mask, action, W, H), wall)):
            if args.skip_torch and name.startswith("torch"):
                continue
            calls = args.calls if name.startswith(("launch", "front")) else max(1, args.calls // 5)
            med, lo, hi = timer(fn, calls, args.repeats)
            row[name + "_us"], row[name + "_us_min"], row[name + "_us_max"] = med * 1e6, lo * 1e6, hi * 1e6
        row["launch_floor_fraction"] = row["floor_us"] / row["launch_device_us"]
        row["launch_tbs"] = row["bytes"] / (row["launch_device_us"] * 1e-6) / 1e12
        if not args.skip_torch:
            row["torch_over_launch"] = row["torch_device_us"] / row["launch_device_us"]
            row["torch_wall_over_front_wall"] = row["torch_wall_us"] / row["front_wall_us"]
        res["shapes"].append(row)
        del got, want, outs
        torch.cuda.empty_cache()
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
