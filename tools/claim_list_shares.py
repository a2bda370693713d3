"""CPU only: the shares of the list claims (pixel_claim.h) on the bench frame, for profiles/claim_lists.txt.

  python tools/claim_list_shares.py [--width 1920 --height 1080 --rows 12 --spp 32]

Runs the host program of tests/cpp/pixel_claim_list_test.cpp over the bench scene and camera, then traces `spp` oracle
samples of every `rows`-th row: the share of pixels with a list, the histogram of list lengths, the share of the rays of
the pixels without a single claim that the per-ray rule settles, and what the others are lost to."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rows", type=int, default=12)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--scene", default="sponza260k")
    ap.add_argument("--why", action="store_true", help="count on stderr why pixels got no list")
    a = ap.parse_args()
    import claim_list_spec as LS
    import oracle_lib as O
    import vermilion_amd as va
    from vermilion_amd import scenes
    pos, nrm, uv = getattr(scenes, a.scene)()
    c = {"sponza260k": scenes.sponza_camera, "cornell8": scenes.cornell_camera, "bunny70k": scenes.bunny_camera,
         "lattice": scenes.lattice_camera}[a.scene]()
    W, H = a.width, a.height
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, 64, back_size=(3.6, 3.6 * H / W))
    osc = O.OracleScene(pos, nrm, uv)
    tree = osc.bvh()
    claims, lists, _, _ = LS.host_lists(pos, tree, [cam], why=a.why)[0]
    flat = claims.reshape(-1)
    n = LS.list_lengths(lists)
    un = flat == LS.NONE
    print("%s %dx%d: single claims %.2f %%, unclaimed %.2f %%" % (a.scene, W, H, 100 * np.mean(~un), 100 * np.mean(un)))
    print("pixels with a list: %.2f %% of all, %.2f %% of the unclaimed" % (100 * np.mean(n > 0), 100 * np.mean(n[un] > 0)))
    for k in range(LS.WORDS + 1):
        print("  list length %d: %.2f %% of the unclaimed" % (k, 100 * np.mean(n[un] == k)))
    rows = np.arange(0, H, a.rows)
    sel = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    sel = sel[un[sel]].astype(np.uint32)
    pix, dirs = LS.sample_rays(cam, sel, a.spp, seed=3, footprint=False)
    _, _, slot, t = LS.host_lists(pos, tree, [cam], rays=[(pix, dirs)])[0]
    bad, settled = LS.verdict(osc, tree, cam, pix, dirs, slot, t)
    print("rows %% %d, %d samples: %d rays of %d unclaimed pixels; settled %.2f %% (of the rays of list pixels: %.2f %%); wrong: %d"
          % (a.rows, a.spp, pix.size, sel.size, 100 * settled / max(pix.size, 1),
             100 * settled / max(int(np.sum(n[pix] > 0)), 1), bad))


if __name__ == "__main__":
    main()
