#!/usr/bin/env python3
"""Place recognition (group (AC)) at the sizes of a drive: descriptors of 20 x 60 over frames of 60 000 rows, and the search of Q = 1 and
16 queries among K = 1 000 and 10 000 keys (HIP events, median of --reps calls after warm-up, min / max beside the median; one process,
the variants of a size timed in alternating rounds).
  (a) us per call of sv_place_descriptor_device (three kernels) for B = 1 and 16 frames, into pre-allocated outputs and workspace;
  (b) us per call of sv_place_match_device (two kernels) with the ring gate off and on - the gate at the tenth part of the keys' ring
      distances -, and with one key per pass instead of four (sv_debug_place), and the byte differences per second of the full search:
      Q x candidates x R S x S over the call's time;
  (c) the same definitions with torch ops on the same device: the descriptor by floor, a [rows, S] table of cross products, bucketize and
      scatter_reduce_("amax"); the search by roll, abs, sum and min over chunks of 1024 keys, the best by a float64 ratio.  Before anything
      is timed their results must equal the kernels'.
The yardstick is never the code under test.  Nothing is asserted about speed.

    timeout -k 10 900 python tools/place_time.py [--reps 21] [--out profiles/place_time.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from warp_time import PKG, alternating  # noqa: E402

ROWS, R, S = 60000, 20, 60


def torch_descriptor(xyz, counts, p, dirs, edge2):
    """stereo_vision.sv.place_descriptor (no weights, no poses) with torch ops -> desc uint8 [B,R,S], ring uint8 [B,R], words int32 [B,4]."""
    B, cap = xyz.shape[:2]
    P = xyz.double()
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    rows = torch.arange(cap, device=xyz.device)[None] < counts.clamp(0, cap)[:, None]
    keep = rows & (x.abs() < p["r_max"]) & (y.abs() < p["r_max"]) & (z >= p["z_lo"]) & (z < p["z_hi"])
    zero = torch.zeros_like(x)
    qx, qy = torch.floor(torch.where(keep, x, zero) / p["unit"]).long(), torch.floor(torch.where(keep, y, zero) / p["unit"]).long()
    d2 = qx * qx + qy * qy
    keep &= (d2 >= p["r_min2"]) & (d2 < 1024 * 1024) & ((qx != 0) | (qy != 0))
    ring = (torch.bucketize(d2, edge2, right=True) - 1).clamp(0, R - 1)
    cross = dirs[:, 0] * qy[..., None] - dirs[:, 1] * qx[..., None]  # [B,cap,S]
    sector = ((cross >= 0) & (cross.roll(-1, 2) < 0)).int().argmax(2)
    code = 1 + torch.floor((torch.where(keep, z, torch.full_like(z, p["z_lo"])) - p["z_lo"]) / p["z_unit"]).long().clamp(max=254)
    at = (torch.arange(B, device=xyz.device)[:, None] * R + ring) * S + sector
    desc = torch.zeros(B * R * S, dtype=torch.long, device=xyz.device).scatter_reduce_(0, at[keep], code[keep], "amax").view(B, R, S)
    words = torch.stack([desc.sum((1, 2)), (desc > 0).sum((1, 2)), keep.sum(1), (rows & ~keep).sum(1)], 1)
    return desc.to(torch.uint8), (desc > 0).sum(2).to(torch.uint8), words.int()


def torch_match(qd, qw, qr, qs, kd, kw, kr, ks, min_gap, ring_gate, chunk=1024):
    """stereo_vision.sv.place_match with torch ops -> best int32 [Q,4], counts int32 [Q,3] (accept 256); the best by a float64 ratio."""
    Q, K = qd.shape[0], kd.shape[0]
    q16, shifts = qd.to(torch.int16), torch.arange(S, device=qd.device)
    word = torch.empty((Q, K), dtype=torch.long, device=qd.device)
    for k0 in range(0, K, chunk):
        k16 = kd[k0:k0 + chunk].to(torch.int16)
        sad = torch.stack([(q16[:, None] - k16.roll(-s, 2)[None]).abs().sum((2, 3), dtype=torch.int32) for s in range(S)], 2)  # [Q,chunk,S]
        word[:, k0:k0 + chunk] = (sad.long() * 256 + shifts).min(2)[0]
    pre = (qw[:, None, 0] > 0) & (kw[None, :, 0] > 0) & ((qs[:, None].long() - ks[None].long()).abs() >= min_gap)
    post = pre & ((qr[:, None].int() - kr[None].int()).abs().sum(2) <= ring_gate) if ring_gate >= 0 else pre
    norm = (qw[:, None, 0] + kw[None, :, 0]).long()
    ratio = torch.where(post, (word >> 8).double() / norm.clamp(min=1).double(), torch.full((Q, K), float("inf"), dtype=torch.float64, device=qd.device))
    at = ratio.argmin(1)
    w, n, some = word.gather(1, at[:, None])[:, 0], norm.gather(1, at[:, None])[:, 0], post.any(1)
    best = torch.stack([torch.where(some, at, -torch.ones_like(at)), torch.where(some, w & 255, 0 * w), torch.where(some, w >> 8, -torch.ones_like(w)), torch.where(some, n, 0 * n)], 1)
    return best.int(), torch.stack([pre.sum(1), post.sum(1), some.long()], 1).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("place_time needs the GPU: nothing is measured without one")
    eng, sv = (importlib.import_module(PKG + "." + m) for m in ("engine", "stereo_vision.sv"))
    p = sv.place_params(40.0, R, S, -1.4, 1.0)
    dirs, edge2 = torch.from_numpy(p["dirs"]).cuda().long(), torch.from_numpy(p["ring_edge2"]).cuda()
    rng = np.random.default_rng(1)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rings": R, "sectors": S, "rows": ROWS}

    for B in (1, 16):
        xyz = rng.uniform(-42, 42, (B, ROWS, 3))
        xyz[..., 2] = rng.uniform(-1.6, 1.2, (B, ROWS))
        xyz, counts = torch.from_numpy(xyz.astype(np.float32)).cuda(), torch.full((B,), ROWS, dtype=torch.int32, device="cuda")
        out = eng.place_descriptor(xyz, None, counts, p)
        ws = torch.empty(B * (4 + R * S), dtype=torch.int32, device="cuda")
        theirs = torch_descriptor(xyz, counts, p, dirs, edge2)
        torch.cuda.synchronize()
        for name, x in zip(("desc", "ring", "words"), theirs):
            if not torch.equal(out[name], x):
                raise SystemExit("the torch form and the kernels disagree on %s at B = %d" % (name, B))
        t = alternating({"call": lambda: eng.place_descriptor(xyz, None, counts, p, out=out, workspace=ws)}, args.reps)
        t.update(alternating({"torch": lambda: torch_descriptor(xyz, counts, p, dirs, edge2)}, args.reps))
        t["call_per_frame_us"] = t["call"]["median_us"] / B
        t["hip_is_faster_than_torch"] = bool(t["call"]["median_us"] < t["torch"]["median_us"])
        t["kept_rows"] = out["words"][:, 2].tolist()[:2]
        res["descriptor_B%d" % B] = t

    for K in (1000, 10000):
        kd = (rng.integers(1, 256, (K, R, S)) * (rng.random((K, R, S)) < 0.3)).astype(np.uint8)
        for Q in (1, 16):
            qd = np.stack([np.roll(kd[rng.integers(0, K)], rng.integers(0, S), axis=1) for _ in range(Q)])
            qd[rng.random(qd.shape) < 0.1] = 0
            dev = []
            for d in (qd, kd):
                occ = (d > 0).sum(2)
                words = np.stack([d.astype(np.int64).sum((1, 2)), occ.sum(1), occ.sum(1), 0 * occ.sum(1)], 1).astype(np.int32)
                dev.append([torch.from_numpy(a).cuda() for a in (d, words, occ.astype(np.uint8))])
            qs, ks = torch.full((Q,), 10 ** 6, dtype=torch.int32, device="cuda"), torch.arange(K, dtype=torch.int32, device="cuda")
            a = dev[0] + [qs] + dev[1] + [ks, 50]
            dist = (dev[0][2][:, None].int() - dev[1][2][None].int()).abs().sum(2)
            gate = int(dist.float().quantile(0.1))
            for name, ring_gate in (("gate_off", -1), ("gate_on", gate)):
                out = eng.place_match(*a, ring_gate=ring_gate)
                ws = torch.empty(8 * Q * ((K + 63) // 64), dtype=torch.int32, device="cuda")
                theirs = torch_match(*a, ring_gate)
                torch.cuda.synchronize()
                for f, x in zip(("best", "counts"), theirs):
                    if not torch.equal(out[f], x):
                        raise SystemExit("the torch form and the kernels disagree on %s at Q = %d, K = %d, %s" % (f, Q, K, name))

                def variant(one_key, ring_gate=ring_gate, out=out, ws=ws, a=a):
                    def run():
                        eng.debug_place(one_key)
                        eng.place_match(*a, ring_gate=ring_gate, out=out, workspace=ws)
                        eng.debug_place(0)
                    return run

                t = alternating({"call": variant(0), "one_key_per_pass": variant(1), "call_again": variant(0)}, args.reps)
                t.update(alternating({"torch": lambda: torch_match(*a, ring_gate)}, max(args.reps // 3, 3) if K * Q > 20000 else args.reps))
                cands = int(out["counts"][:, 1].sum())
                t["candidates"], t["ring_gate"] = cands, ring_gate
                t["byte_differences"] = cands * R * S * S
                t["tera_byte_differences_per_s"] = t["byte_differences"] / t["call"]["median_us"] / 1e6
                t["hip_is_faster_than_torch"] = bool(t["call"]["median_us"] < t["torch"]["median_us"])
                res["match_Q%d_K%d_%s" % (Q, K, name)] = t
    res["not_measured"] = "kernel times by a profiler trace; descriptors other than 20 x 60; K above 10 000; f64 rows; rows under poses"
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
