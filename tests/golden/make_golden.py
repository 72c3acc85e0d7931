"""Generates the committed golden fixtures from the REFERENCE ITSELF (oracle/_ref/libelas_ref.so, i.e. the
reference's serial LIBELAS compiled from /root/reference by oracle/Makefile), run in its canonical state
(zero-filled scratch, IEEE flags).  Only runs in the build container:

    python tests/golden/make_golden.py                  # everything
    python tests/golden/make_golden.py --extra-inputs   # only the input images of tests/test_oracle_vs_ref.py (+ ref_digests.json)
    python tests/golden/make_golden.py --ref-digests    # only ref_digests.json (the reference's results of that module's cases)

Fixtures are data only: gray input images and the arrays / digests the reference produced for them.
Gray conversion of the bundled KITTI colour PNGs uses the OpenCV-4.x 15-bit BGR2GRAY weights the reference
driver would apply (stereo_vision.cpp:338-339).
"""
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from pyoracle import ElasParams, RefElas  # noqa: E402

REF = "/root/reference"
STAGES = ["desc1", "desc2", "dcan_raw", "support", "tri1", "tri2", "planes1", "planes2", "grid1", "grid2",
          "wta1", "wta2", "lr1", "lr2", "speckle1", "speckle2", "gap1", "gap2", "amean1", "amean2", "final1", "final2"]


def gray_cv4(path):
    a = np.asarray(Image.open(path).convert("RGB")).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    return ((b * 3735 + g * 19235 + r * 9798 + 16384) >> 15).astype(np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def params_for(case):
    if case["preset"] == "driver":
        return ElasParams.driver(case["disp_max"])
    p = ElasParams.preset(case["preset"])
    p.disp_max = case["disp_max"]
    return p


def with_sub(p, case):
    p.subsampling = 1 if case.get("subsampling") else 0  # half-resolution mode (elas.h:83-85)
    p.disp_min = int(case.get("disp_min", 0))            # first disparity of the support search (elas.h:61, elas.cpp:318)
    return p


KITTI_MINI_FRAMES = 21  # image_02 / image_03 pairs of datasets/kitti_mini
PROFILE_PAIRS = ["aloe", "cones", "raindeer", "urban1", "urban2", "urban3", "urban4"]  # datasets/profile


def extra_inputs():
    """Input images only, for tests/test_oracle_vs_ref.py: the kitti_mini frames main() does not write (gray, kitti<f>_*.png,
    digests of the frames without an entry in digests.json are not needed) and the datasets/profile pairs as lossless PNGs."""
    for f in range(KITTI_MINI_FRAMES):
        if os.path.exists(os.path.join(HERE, "kitti%d_left.png" % f)):
            continue
        for cam, side in (("image_02", "left"), ("image_03", "right")):
            g = gray_cv4(REF + "/datasets/kitti_mini/%s/data/%010d.png" % (cam, f))
            Image.fromarray(g).save(os.path.join(HERE, "kitti%d_%s.png" % (f, side)), optimize=True)
    for name in PROFILE_PAIRS:
        for side in ("left", "right"):
            a = np.asarray(Image.open(REF + "/datasets/profile/%s_%s.pgm" % (name, side)))
            Image.fromarray(a).save(os.path.join(HERE, "profile_%s_%s.png" % (name, side)), optimize=True)


def ref_digests():
    """ref_digests.json: the reference's side of tests/test_oracle_vs_ref.py - sha256 of every stage for each case the test
    module generates (and of the triangles / maps where it compares those) - so that the test needs no oracle/_ref."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_oracle_vs_ref as t

    ref, out = RefElas(), {}
    cases = [t.synthetic_case(*c, preset) for c in t.SYNTHETIC for preset in t.PRESETS] + list(t.noise_cases())
    cases += [t.kitti_mini_case(f) for f in t.KITTI_MINI_FRAMES] + [t.profile_case(n, pr) for n in t.PROFILE_PAIRS for pr in ("robotics", "middlebury")]
    driver, (key, p, L, R) = t.textureless_cases()
    for k, p_, L_, R_ in cases + [driver]:
        out[k] = t.stage_digests(ref, p_, L_, R_)
    D1, D2, _ = ref.process(p, L, R)
    out[key] = [sha(D1), sha(D2)]
    out["delaunay_random_sets"] = {str(it): [int(a.shape[0]), sha(a)] for it, _, _, xy in t.delaunay_sets() for a in [ref.delaunay(xy)]}
    import degenerate_sets as ds
    out["delaunay_structured_sets"] = {name: [int(a.shape[0]), sha(a)] for name, xy in ds.sets() for a in [ref.delaunay(xy.astype(np.float32))]}
    for case in ds.pair_cases():
        k, p_, L_, R_, by_ref = t.degenerate_pair_case(case[0])
        if by_ref:
            lib = ref
        else:  # (a pair the compiled reference cannot run: the restatement's own result, under a key that says so)
            from pyoracle import Oracle
            lib = Oracle()
        out[k] = t.stage_digests(lib, p_, L_, R_)
        out[k]["triangles"] = [int(lib.stage("tri1").size // 3), int(lib.stage("tri2").size // 3)]
    for k, _, p_, L_, R_ in t.random_parameter_cases():
        n = ref.run_stages(p_, L_, R_)
        out[k] = t.stage_digests(ref, p_, L_, R_) if n >= 3 else {"n": n}
    import content_cases as cc
    for key in cc.keys():
        k, p_, L_, R_ = t.content_case(key)
        n = ref.run_stages(p_, L_, R_)
        out[k] = {"n": n, "stages": {s: sha(ref.stage(s)) for s in (STAGES if n >= 3 else t.CONTENT_EARLY_STAGES)}}
    with open(os.path.join(HERE, "ref_digests.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def main():
    sys.path.insert(0, ROOT)
    import importlib
    synth = importlib.import_module("low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd.synth")
    ref = RefElas()
    k0l = gray_cv4(REF + "/datasets/kitti_mini/image_02/data/0000000000.png")
    k0r = gray_cv4(REF + "/datasets/kitti_mini/image_03/data/0000000000.png")
    Image.fromarray(k0l).save(os.path.join(HERE, "kitti0_left.png"), optimize=True)
    Image.fromarray(k0r).save(os.path.join(HERE, "kitti0_right.png"), optimize=True)
    # colour crop of pair 0 (the region of the kitti0_crop cases): input of the BGRA -> gray test of the legacy entry point
    for side, cam in (("left", "image_02"), ("right", "image_03")):
        rgb = np.asarray(Image.open(REF + "/datasets/kitti_mini/%s/data/0000000000.png" % cam).convert("RGB"))[150:278, 400:720].copy()
        Image.fromarray(rgb).save(os.path.join(HERE, "kitti0_crop_color_%s.png" % side), optimize=True)
    cl = np.asarray(Image.open(REF + "/datasets/profile/cones_left.pgm"))[200:500, 300:700].copy()
    cr = np.asarray(Image.open(REF + "/datasets/profile/cones_right.pgm"))[200:500, 300:700].copy()
    Image.fromarray(cl).save(os.path.join(HERE, "cones_crop_left.png"), optimize=True)
    Image.fromarray(cr).save(os.path.join(HERE, "cones_crop_right.png"), optimize=True)

    more = {}
    for f in (3, 7, 10, 13, 17, 20):  # more frames of the sequence (digests only): real maps are far more fragmented than the synthetic pairs;
        # frames 13, 17 and 20 have the corner support point with disparity 0 twice (coincident vertices for the triangulation)
        gl = gray_cv4(REF + "/datasets/kitti_mini/image_02/data/%010d.png" % f)
        gr = gray_cv4(REF + "/datasets/kitti_mini/image_03/data/%010d.png" % f)
        Image.fromarray(gl).save(os.path.join(HERE, "kitti%d_left.png" % f), optimize=True)
        Image.fromarray(gr).save(os.path.join(HERE, "kitti%d_right.png" % f), optimize=True)
        more["kitti%d" % f] = (gl, gr)
    images = {
        "kitti0": (k0l, k0r),
        "kitti0_crop": (k0l[150:278, 400:720].copy(), k0r[150:278, 400:720].copy()),
        "cones_crop": (cl, cr),
    }
    images.update(more)
    cases = [
        dict(name="kitti0_d64", image="kitti0", preset="driver", disp_max=63, keep=["support", "tri1", "tri2", "wta1", "wta2", "final1"]),
        dict(name="kitti0_d128", image="kitti0", preset="driver", disp_max=127,
             keep=["support", "tri1", "tri2", "planes1", "planes2", "wta1", "wta2", "lr1", "speckle1", "gap1", "amean1", "final1"]),
        dict(name="kitti0_d256", image="kitti0", preset="driver", disp_max=255, keep=["support", "tri1", "tri2", "wta1", "wta2", "final1"]),
        dict(name="kitti3_d128", image="kitti3", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti7_d128", image="kitti7", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti10_d128", image="kitti10", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti13_d128", image="kitti13", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti17_d128", image="kitti17", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti20_d128", image="kitti20", preset="driver", disp_max=127, keep=[]),
        dict(name="kitti0_d256_sub", image="kitti0", preset="driver", disp_max=255, subsampling=1, keep=[]),
        dict(name="kitti0_crop_d64", image="kitti0_crop", preset="driver", disp_max=63, keep=STAGES),
        # disp_min > 0 (elas.h:61): the support matching's search starts there (elas.cpp:318-330), nothing else uses it
        dict(name="kitti0_crop_d64_dmin6", image="kitti0_crop", preset="driver", disp_max=63, disp_min=6, keep=["support", "wta1", "final1"]),
        dict(name="kitti0_d128_dmin20", image="kitti0", preset="driver", disp_max=127, disp_min=20, keep=[]),
        dict(name="cones_crop_robotics", image="cones_crop", preset="robotics", disp_max=63, keep=["support", "tri1", "tri2", "wta1", "wta2", "final1"]),
        dict(name="cones_crop_middlebury", image="cones_crop", preset="middlebury", disp_max=63, keep=["support", "wta1", "final1", "final2"]),
        dict(name="synth1000_d128", synth=dict(seed=1000, H=375, W=1242, D=128), preset="driver", disp_max=127, keep=[]),
        dict(name="synth7_d64", synth=dict(seed=7, H=120, W=320, D=64), preset="driver", disp_max=63, keep=["support", "tri1", "tri2", "wta1", "final1"]),
        dict(name="synth8_d32", synth=dict(seed=8, H=97, W=203, D=32), preset="driver", disp_max=31, keep=["support", "wta1", "final1"]),
        # half-resolution mode (Elas::parameters::subsampling): maps are (W/2) x (H/2)
        dict(name="kitti0_d128_sub", image="kitti0", preset="driver", disp_max=127, subsampling=1,
             keep=["support", "tri1", "tri2", "wta1", "wta2", "lr1", "speckle1", "gap1", "amean1", "final1"]),
        dict(name="kitti0_crop_d64_sub", image="kitti0_crop", preset="driver", disp_max=63, subsampling=1, keep=STAGES),
        dict(name="cones_crop_robotics_sub", image="cones_crop", preset="robotics", disp_max=63, subsampling=1, keep=["support", "wta1", "final1", "final2"]),
        dict(name="synth8_d32_sub", synth=dict(seed=8, H=97, W=203, D=32), preset="driver", disp_max=31, subsampling=1, keep=["support", "wta1", "final1"]),
        dict(name="synth5000_4kstrip_d192", synth=dict(seed=5000, H=512, W=3840, D=192, scale=3), preset="driver", disp_max=191, keep=[]),
        # BASELINE.json configs[4] at full size (digest only): the pair bench.py's parity gate of the 4K configuration runs
        dict(name="synth5000_4k_d192", synth=dict(seed=5000, H=2160, W=3840, D=192, scale=3), preset="driver", disp_max=191, keep=[]),
    ]
    digests = {}
    for case in cases:
        if "synth" in case:
            L, R = synth.make_pair(**case["synth"])
        else:
            L, R = images[case["image"]]
        p = with_sub(params_for(case), case)
        n = ref.run_stages(p, L, R)
        st = {k: ref.stage(k) for k in STAGES}
        entry = {"n_support": int(n), "shape": [int(L.shape[0]), int(L.shape[1])], "preset": case["preset"], "disp_max": case["disp_max"],
                 "input_sha256": [sha(L), sha(R)], "stages": {k: sha(v) for k, v in st.items()}}
        if case.get("subsampling"):
            entry["subsampling"] = 1
        if case.get("disp_min"):
            entry["disp_min"] = int(case["disp_min"])
        if "synth" in case:
            entry["synth"] = case["synth"]
        else:
            entry["image"] = case["image"]
        digests[case["name"]] = entry
        if case["keep"]:
            arrs = {}
            for k in case["keep"]:
                v = st[k]
                if k.startswith("wta"):
                    v = v.astype(np.int16)  # integer-valued: -10, -1, 0..disp_max
                arrs[k] = v
            np.savez_compressed(os.path.join(HERE, case["name"] + ".npz"), **arrs)
        print(case["name"], "n_support", n, "tris", st["tri1"].size // 3, st["tri2"].size // 3)
    with open(os.path.join(HERE, "digests.json"), "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    if "--extra-inputs" not in sys.argv and "--ref-digests" not in sys.argv:
        main()
    if "--ref-digests" not in sys.argv:
        extra_inputs()
    ref_digests()
