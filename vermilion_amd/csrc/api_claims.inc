// api_claims.inc — part of vmx_api.cpp: the per-pixel claims and list claims of a run's camera (pixel_claim.h) — build_claims,
// which render_bind calls, and the entries that read the tables and the routes' counters back
namespace {

// Claims pay from this many samples per pixel on: below it a run builds none.  Measured on the 1080p headline frame,
// claims on against off (profiles/pixel_claims.txt section 6): +1.17 ms at 16 samples, +0.11 at 32, -2.21 at 64, -5.99 at
// 128 — 64 is the smallest of the swept values at which claims are not slower.
constexpr uint32_t kClaimMinSamples = 64;
uint32_t claim_min_samples() {
#ifdef VMX_AB_KERNELS  // A/B library only: VMX_CLAIM_MIN_SPP overrides the threshold (tools/claim_sweep.py measures below it)
    if (const char *e = std::getenv("VMX_CLAIM_MIN_SPP")) {
        const unsigned long v = std::strtoul(e, nullptr, 10);
        if (v) return (uint32_t)std::min<unsigned long>(v, 0xFFFFFFFFul);
    }
#endif
    return kClaimMinSamples;
}

// the per-pixel claims of the frame `fr` from the camera tables in the workspace, into ws.claims[0, npix) and the number
// of claimed pixels into ws.claims[npix]; lists: the list records of the pixels without a claim into ws.claim_lists too, in
// a second launch: k_pixel_claims settles the claims and the empty records and marks, per 8 x 8 tile, the pixels whose
// list is still to be made; those are listed in tile order on the device (the scan of the live list) and k_pixel_lists
// walks for them in full waves.  The list's length stays on the device: nothing here waits for the stream.
int build_claims(vmx_scene *sc, const FrameDev &fr, const Tuning &tn, uint32_t npix, bool lists, hipStream_t s) {
    Workspace &ws = sc->ws;
    if (ws.claims.ensure((size_t)npix + 2)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the pixel claims");  // (+ the count, + the claim kernel's work head)
    if (lists && ws.claim_lists.ensure((size_t)npix * kListWords)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the claim lists");
    WorkDev wk = make_work(nullptr, nullptr);
    wk.cam_inner = ws.cam_inner.p, wk.cam_tris = ws.cam_inner.p + std::max<size_t>(sc->n_inner, 1) * 64 * 8;
    const uint64_t tiles = (uint64_t)((fr.width + 7u) / 8u) * ((fr.local_rows + 7u) / 8u);
    if (tiles * 64 > 0xFFFFFFFFull) return fail(VMX_ERR_INVALID, "frame too large for the pixel claims");
    // both kernels run on a resident grid and hand out their work on the device
    int cblocks = 0;
    HIP_TRY((hipError_t)query_pixel_claims_blocks_per_cu(kPathsBlock, (kPathsBlock / 64) * (tn.lds_primary + 1) * 512, &cblocks));
    if (cblocks < 1) return fail(VMX_ERR_HIP, "kernel does not fit on a CU (LDS stack too deep?)");
    LaunchCfg cfg = paths_cfg(sc, tn.lds_primary, tiles * 64, cblocks);
    LaunchCfg lcfg = cfg;
    size_t tmp_bytes = 0;
    if (lists) {
        // the list kernel's grid, or less for a frame with fewer pixels than that; the
        // stack binding (LDS levels, overflow slab) is the claim kernel's, sized for the larger of the two grids
        int blocks = 0;
        HIP_TRY((hipError_t)query_pixel_lists_blocks_per_cu(kPathsBlock, cfg.lds_bytes, &blocks));
        if (blocks < 1) return fail(VMX_ERR_HIP, "kernel does not fit on a CU (LDS stack too deep?)");
        lcfg = paths_cfg(sc, tn.lds_primary, (uint64_t)npix, blocks);
        tmp_bytes = live_compact_tmp_bytes((uint32_t)tiles);
        if (ws.claim_pend_mask.ensure(tiles) || ws.claim_pend_u32.ensure(2 * tiles + 2) || ws.claim_pend_ids.ensure(npix) ||
            ws.claim_pend_tmp.ensure(tmp_bytes + 256))
            return fail(VMX_ERR_NOMEM, "hipMalloc failed for the list of pixels without a claim");
    }
    int rc = bind_stack(sc, tn, tn.lds_primary, std::max(cfg.grid, lcfg.grid), tiles * 64, wk);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ws.claims.p + npix, 0, 8, s));
    if (!lists) {
        LAUNCH_TRY(launch_pixel_claims(sc->dev, fr, wk, ws.claims.p, nullptr, ws.claims.p + npix, nullptr, nullptr, cfg, s));
    } else {
        unsigned int *cnt = ws.claim_pend_u32.p, *offs = cnt + tiles, *len = offs + tiles, *head = len + 1;
        LAUNCH_TRY(launch_pixel_claims(sc->dev, fr, wk, ws.claims.p, ws.claim_lists.p, ws.claims.p + npix, ws.claim_pend_mask.p, cnt, cfg, s));
        HIP_TRY(hipMemsetAsync(len, 0, 8, s));  // (the list's length and the list kernel's work head)
        HIP_TRY((hipError_t)launch_live_compact(ws.claim_pend_mask.p, cnt, (uint32_t)tiles, offs, ws.claim_pend_ids.p, len,
                                                ws.claim_pend_tmp.p, tmp_bytes, (uint32_t)sc->num_cus, s));
        LAUNCH_TRY(launch_pixel_lists(sc->dev, fr, wk, ws.claim_pend_ids.p, len, head, ws.claim_lists.p, lcfg, s));
    }
    return VMX_OK;
}

}  // namespace

extern "C" {

static int pixel_claims_impl(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t *claims_out,
                             uint32_t *lists_out, uint32_t *n_claimed) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !cam || !opts) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    int rc = bind_device(sc);
    if (rc) return rc;
    FrameDev fr;
    if ((rc = make_frame(*cam, *opts, fr))) return rc;
    const uint32_t npix = fr.width * fr.local_rows;
    if (n_claimed) *n_claimed = 0;
    if (npix == 0) return VMX_OK;
    Workspace &ws = sc->ws;
    hipStream_t s = sc->stream;
    if ((rc = sc->upd.done.wait(s))) return rc;
    const size_t n_inner = std::max<size_t>(sc->n_inner, 1);
    if (ws.cam_inner.ensure(n_inner * 64 * 8 + (size_t)sc->ntris * 64)) return fail(VMX_ERR_NOMEM, "hipMalloc failed for the camera tables");
    LAUNCH_TRY(launch_camera_tables(sc->dev, sc->n_inner, fr.px, fr.py, fr.pz, ws.cam_inner.p, ws.cam_inner.p + n_inner * 64 * 8, (uint32_t)sc->num_cus, s));
    if ((rc = build_claims(sc, fr, make_tuning(sc, opts), npix, lists_out != nullptr, s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (claims_out) HIP_TRY(hipMemcpy(claims_out, ws.claims.p, (size_t)npix * 4, hipMemcpyDeviceToHost));
    if (lists_out) HIP_TRY(hipMemcpy(lists_out, ws.claim_lists.p, (size_t)npix * kListWords * 4, hipMemcpyDeviceToHost));
    if (n_claimed) HIP_TRY(hipMemcpy(n_claimed, ws.claims.p + npix, 4, hipMemcpyDeviceToHost));
    return VMX_OK;
}

int vmx_pixel_claims(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t *claims_out,
                     uint32_t *n_claimed) {
    return pixel_claims_impl(csc, cam, opts, claims_out, nullptr, n_claimed);
}

int vmx_pixel_claim_lists(const vmx_scene *csc, const vmx_camera *cam, const vmx_opts *opts, uint32_t *claims_out,
                          uint32_t *lists_out, uint32_t *n_claimed) {
    if (!lists_out) return fail(VMX_ERR_INVALID, "NULL argument");
    return pixel_claims_impl(csc, cam, opts, claims_out, lists_out, n_claimed);
}

int vmx_list_settled_rays(const vmx_scene *csc, uint64_t *rays) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !rays) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *rays = sc->list_settled;
    return VMX_OK;
}

int vmx_fused_camera_paths(const vmx_scene *csc, uint64_t *paths) {
    vmx_scene *sc = const_cast<vmx_scene *>(csc);
    if (!sc || !paths) return fail(VMX_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lock(sc->mu);
    *paths = sc->fused_paths;
    return VMX_OK;
}

} /* extern "C" */
