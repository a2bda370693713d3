"""Per-pixel claims (pixel_claim.h) against the samples per pixel: the 1080p bench frame in the headline form at 16 ... 256
spp, fixed count, claims forced on (the A/B library, `make ab`, reads VMX_CLAIM_MIN_SPP) against claims off (reserved[0] bit 11):
device time of the frame, of the claim kernel and of the camera traversal, best of three.  The smallest spp at which
"on" is not slower is the threshold kClaimMinSamples (api_claims.inc)."""
import os, sys
os.environ.setdefault("VMX_CLAIM_MIN_SPP", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, vermilion_amd as va
from vermilion_amd import scenes, _lib
AB = _lib.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "build", "libvermilion_hip_ab.so"))
pos, nrm, uv = scenes.sponza260k(); c = scenes.sponza_camera()
W, H = 1920, 1080
sc = va.Scene(pos, nrm, uv, lib=AB)
out = torch.empty((H, W, 5), device="cuda")
for spp in (16, 32, 64, 128, 256):
    cam = va.make_camera(c["position"], c["rotation_deg"], W, H, spp, back_size=(3.6, 3.6 * H / W))
    row = []
    for off in (0, 0x800):
        o = va.make_opts(seed=1, early_stop=False, pipeline=4 | 0x100 | off)
        best = None
        for _ in range(4):  # the first one warms up
            st = sc.render_device(cam, o, out.data_ptr()); torch.cuda.synchronize()
            t = sc.timings()
            if best is None or st["ms_device"] < best[0]:
                best = (st["ms_device"], t["other"]["ms"], t["trace_camera"]["ms"])
        row.append(best)
    (on, ck, tc_on), (offm, _, tc_off) = row
    print(f"spp {spp:3d}: frame on {on:7.2f} ms / off {offm:7.2f} ms ({on - offm:+.2f}) | claim kernel {ck:.2f} ms | trace_camera on {tc_on:.2f} / off {tc_off:.2f} ms", flush=True)
