#!/usr/bin/env python3
"""Object links (group (AB)) on the committed KITTI frames at full size, 1242 x 375, pair kitti0 -> 1 with the engine's own maps, objects'
boxes and flow_match's matches at step 8, for B = 1 and B = 16 pairs (HIP events, median of --reps calls after warm-up, min / max beside
the median; one process, the variants of a batch size timed in alternating rounds, the full call at both ends of a round).
  (a) us per call of sv_object_links_device (four kernels: clear, votes, link, sums) into pre-allocated outputs and workspace;
  (b) the same call with kernels left out from the end through sv_debug_object_links - clear alone, clear + votes, clear + votes + link -,
      so each kernel's share is a difference of medians;
  (c) the same definition with torch ops on the same device: the membership as boolean [n, M] tables, the votes by a float64 matmul (exact:
      below 2^53), the link by packed keys and scatter_reduce_("amax"), the doubles in float64 tensors, the sums by an int64 product summed
      over the matches.  Before anything is timed its votes, link and sums must equal the kernels' bit for bit;
  (d) StereoRig.track of the four frames per frame beside StereoRig.odometry per frame, by the host's clock around a synchronise.
The yardstick is never the code under test.  Nothing is asserted about speed.

    timeout -k 10 600 python tools/object_links_time.py [--reps 21] [--out profiles/object_links_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from warp_time import YML, PKG, alternating, host_clock  # noqa: E402

WORDS = dict(band_q=48, min_votes=3, share=128)


def torch_links(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, cam, W, H, band_q, min_votes, share):
    """stereo_vision.sv.object_links (no gate) with torch ops on the tensors' device -> votes int32 [B,M,M+1], link int32 [B,M,4], sums
    int64 [B,M,16]."""
    B, cap = matches.shape[:2]
    M = boxes0.shape[1]
    dev = matches.device
    m = matches.long()
    u0, v0, d0, u1, v1, d1 = (m[..., k] for k in range(6))
    rows = torch.arange(cap, device=dev)[None] < counts.clamp(0, cap)[:, None].long()
    live = rows & (d0 >= 1) & (d0 <= 2 ** 20)
    idx = torch.arange(M, device=dev)

    def members(u, v, d, boxes, n, q, needs_d):
        b = boxes.long()
        cl = lambda a, size: a.clamp(0, size - 1)  # noqa: E731
        x0, x1, y0, y1 = cl(b[..., 0], W), cl(b[..., 0] + b[..., 2], W), cl(b[..., 1], H), cl(b[..., 1] + b[..., 3], H)
        ok = (u[..., None] >= x0[:, None]) & (u[..., None] < x1[:, None]) & (v[..., None] >= y0[:, None]) & (v[..., None] < y1[:, None])
        ok &= (idx[None] < n.clamp(0, M)[:, None].long())[:, None]
        near = (d[..., None] - 4 * q.long()[:, None]).abs() <= band_q
        if needs_d:
            near &= d[..., None] > 0
        return ok & ((q[:, None] <= 0) | near)

    in0 = members(u0, v0, d0, boxes0, n0, q0, False) & live[..., None]  # [B,cap,M]
    in1 = members(u1, v1, d1, boxes1, n1, q1, True)
    votes = torch.cat([torch.matmul(in0.double().transpose(1, 2), in1.double()), in0.double().sum(1)[..., None]], 2).long()  # [B,M,M+1]
    vj = votes[..., :M]
    key = vj * 64 + (63 - idx)
    best_key, _ = key.max(2)
    best, bj = best_key >> 6, 63 - (best_key & 63)
    second = vj.masked_fill(idx[None, None] == bj[..., None], 0).max(2)[0] if M > 1 else torch.zeros_like(best)
    members_n = votes[..., M]
    keep = (best >= min_votes) & (256 * best >= share * members_n)
    claim = torch.where(keep, best * 64 + (63 - idx[None]), torch.full_like(best, -1))
    top = torch.full((B, M), -1, dtype=torch.long, device=dev).scatter_reduce_(1, bj, claim, "amax")
    won = keep & (top.gather(1, bj) == claim)
    link = torch.stack([torch.where(won, bj, torch.full_like(bj, -1)), best, members_n, second], 2)

    both = live & (d1 >= 1) & (d1 <= 2 ** 20)
    d0s, d1s = torch.where(live, d0, torch.ones_like(d0)).double(), torch.where(both, d1, torch.ones_like(d1)).double()
    X0 = (((u0.double() - cam["cx"]) * cam["b16"]) / d0s, ((v0.double() - cam["cy"]) * cam["b16"]) / d0s, cam["fb16"] / d0s)
    X1 = (((u1.double() - cam["cx"]) * cam["b16"]) / d1s, ((v1.double() - cam["cy"]) * cam["b16"]) / d1s, cam["fb16"] / d1s)
    P = poses.view(B, 12, 1)
    Xc = [((P[:, 3 * k] * X0[0] + P[:, 3 * k + 1] * X0[1]) + P[:, 3 * k + 2] * X0[2]) + P[:, 9 + k] for k in range(3)]
    ok = both & (Xc[2] > 0.1)
    zs = torch.where(ok, Xc[2], torch.ones_like(Xc[2]))
    pu = torch.floor(16.0 * (cam["f"] * (Xc[0] / zs) + cam["cx"]) + 0.5)
    pv = torch.floor(16.0 * (cam["f"] * (Xc[1] / zs) + cam["cy"]) + 0.5)
    pd = torch.floor(16.0 * (cam["fb"] / zs) + 0.5)
    inside = ok & (pu.abs() <= 2 ** 30) & (pv.abs() <= 2 ** 30) & (pd.abs() <= 2 ** 30)
    zero = torch.zeros_like(pu)
    q = lambda v, lim: torch.floor(torch.where(inside, v, zero) + 0.5).clamp(-lim, lim).long()  # noqa: E731
    r = [(16 * u1 - torch.where(inside, pu, zero).long()).clamp(-2 ** 20, 2 ** 20), (16 * v1 - torch.where(inside, pv, zero).long()).clamp(-2 ** 20, 2 ** 20),
         (d1 - torch.where(inside, pd, zero).long()).clamp(-2 ** 20, 2 ** 20)]
    mv = [q(1024.0 * (X1[a] - Xc[a]), 2 ** 20) for a in range(3)]
    pq = [q(1024.0 * X1[a], 2 ** 30) for a in range(3)]
    one = torch.ones_like(u0)
    vals = torch.stack([one, one, r[0], r[1], r[2], r[0] * r[0] + r[1] * r[1]] + mv + [x * x for x in mv] + pq + [torch.zeros_like(u0)], 2)  # [B,cap,16]
    to = torch.where(won, bj, torch.zeros_like(bj))  # [B,M]
    fed = in0 & in1.gather(2, to[:, None].expand(B, cap, M)) & won[:, None] & inside[..., None]  # [B,cap,M]
    sums = torch.stack([(fed[b, :, :, None] * vals[b, :, None, :]).sum(0) for b in range(B)])
    return votes.int(), link.int(), sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("object_links_time needs the GPU: nothing is measured without one")
    eng, rigmod, sv = (importlib.import_module(PKG + "." + m) for m in ("engine", "rig", "stereo_vision.sv"))
    golden = os.path.join(ROOT, "tests", "golden")
    ls = np.stack([np.repeat(np.asarray(Image.open(os.path.join(golden, "kitti%d_left.png" % k)))[..., None], 3, -1) for k in range(4)])
    rs = np.stack([np.repeat(np.asarray(Image.open(os.path.join(golden, "kitti%d_right.png" % k)))[..., None], 3, -1) for k in range(4)])
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "rectified.yml"), "w") as f:
            f.write(YML)
        rig = rigmod.StereoRig(1242, 375, calibration=os.path.join(tmp, "rectified.yml"), params=eng.SvParams.driver(127))
    left, right = torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda()
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "frames": "kitti0..3, 1242 x 375, disp_max 127", "words": dict(WORDS, gate_m=256, step=8)}
    try:
        got = rig.track(left, right)
        if not got["ok"].all():
            raise SystemExit("the odometry of the four frames did not fit")
        camera = rig.render_camera(1.0)
        cam = sv.flow_camera(camera)
        n_host, linked = got["n"].cpu().numpy(), got["link"].cpu().numpy()[..., 0] >= 0
        res["objects_per_frame"], res["left_out"] = n_host.tolist(), got["left_out"].tolist()
        res["linked_per_pair"] = linked.sum(1).tolist()
        res["matches_per_pair"] = got["matches"]["counts"].cpu().numpy().tolist()
        res["link_rows_per_pair"] = [got["link"][k, :n_host[k]].cpu().numpy().tolist() for k in range(3)]  # (j or -1, votes, members, second) per object
        res["motions_m_per_frame"] = [[int(k), int(i), int(got["count"][k, i])] + np.round(got["motion"][k, i], 3).tolist() for k, i in zip(*np.nonzero(linked)) if got["count"][k, i] >= 8]
        M = int(got["boxes"].shape[1])
        q = got["stat"][:, :, 2].contiguous()
        for B in (1, 16):
            rep = lambda t: t[0:1].repeat(B, *([1] * (t.dim() - 1))).contiguous()  # noqa: E731 (kitti0 -> 1, B times)
            a = dict(matches=rep(got["matches"]["matches"]), counts=rep(got["matches"]["counts"]), poses=torch.from_numpy(np.tile(got["rel"][0:1], (B, 1))).cuda(),
                     boxes0=rep(got["boxes"][0:1]), n0=rep(got["n"][0:1]), q0=rep(q[0:1]), boxes1=rep(got["boxes"][1:2]), n1=rep(got["n"][1:2]), q1=rep(q[1:2]))
            cap = int(a["matches"].shape[1])
            call = lambda **kw: eng.object_links(*a.values(), camera, 1242, 375, **WORDS, **kw)  # noqa: E731
            out = call()
            ws = torch.empty(2 * B * cap, dtype=torch.int64, device="cuda")
            theirs = torch_links(*a.values(), cam, 1242, 375, **WORDS)
            torch.cuda.synchronize()
            for name, x in zip(("votes", "link", "sums"), theirs):
                if out[name].dtype != x.dtype or not torch.equal(out[name], x):
                    raise SystemExit("the torch form and the kernels disagree on %s at B = %d" % (name, B))

            def variant(stop=0):
                def run():
                    eng.debug_object_links(stop)
                    call(out=out, workspace=ws)
                    eng.debug_object_links()
                return run

            # the torch form is timed on its own: what runs right behind it pays for the memory it frees; "call_again" shows what the place in a round is worth
            t = alternating({"call": variant(), "clear_only": variant(3), "clear_votes": variant(2), "clear_votes_link": variant(1),
                             "call_again": variant()}, args.reps)
            t.update(alternating({"torch": lambda: torch_links(*a.values(), cam, 1242, 375, **WORDS)}, args.reps))
            call(out=out, workspace=ws)  # the outputs of the full call again
            med = lambda k: t[k]["median_us"]  # noqa: E731
            t["by_difference_us"] = {"clear": med("clear_only"), "votes": med("clear_votes") - med("clear_only"), "link": med("clear_votes_link") - med("clear_votes"),
                                     "sums": med("call_again") - med("clear_votes_link")}
            t["call_per_frame_us"] = med("call") / B
            t["hip_is_faster_than_torch"] = bool(med("call") < med("torch"))
            t["matches"], t["capacity"], t["max_boxes"] = int(a["counts"][0]), cap, M
            t["linked"], t["fed_matches"] = int((out["link"][0, :, 0] >= 0).sum()), int(out["sums"][0, :, 0].sum())
            res["B%d" % B] = t
        reps = max(args.reps // 3, 3)
        tr, od = host_clock(lambda: rig.track(left, right), reps), host_clock(lambda: rig.odometry(left, right), reps)
        ob = host_clock(lambda: rig.objects(left, right), reps)
        res["track_per_frame"], res["odometry_per_frame"], res["objects_per_frame_us"] = ({k: x / 4.0 for k, x in v.items()} for v in (tr, od, ob))
        res["track_adds_to_odometry_us_per_frame"] = res["track_per_frame"]["median_us"] - res["odometry_per_frame"]["median_us"]
        res["not_measured"] = "kernel times by a profiler trace; B between 1 and 16; boxes from a detector; more than the 4 committed frames"
    finally:
        rig.close()
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
