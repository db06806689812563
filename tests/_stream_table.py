"""TEST INFRASTRUCTURE: the table of tests/test_gpu_streams.py as plain data -- every prototype of include/tomo_mi355x.h
that takes a `void *stream`, the case of that file that runs it on a side stream behind a delay, and what INTEGRATION.md
promises about it.  tests/test_stream_coverage.py holds the table to the header and to the document without a GPU; nothing
here imports torch.

ASYNC   asynchronous on the stream passed in: after the call returns the case asserts that the stream is still busy
SYNC    returns a scalar to the host or keeps a per-call workspace: the call waits for its stream; values only
TOL     takes a tolerance: asynchronous with a tolerance of 0 -- what its case asserts --, waits at every check with one > 0
        (the cases of the two *_tol entries run that as well, values only)"""

ASYNC, SYNC, TOL = "asynchronous", "synchronising", "asynchronous unless its tolerance is > 0"

# the entry points of the third kind (the kind of a case below is what the case asserts after its calls)
TOL_ENTRIES = ["tomo_pdtv_tol", "tomo_roftv_tol", "tomo_pdtv_slices", "tomo_roftv_slices", "tomo_tgv", "tomo_ndf", "tomo_diff4th",
               "tomo_llt_rof", "tomo_nltv"]

# case of tests/test_gpu_streams.py -> (kind, the entry points it runs)
CASES = {
    "projector_pair": (ASYNC, ["tomo_fp3d", "tomo_bp3d", "tomo_bp3d_matched"]),
    "fused_residuals": (ASYNC, ["tomo_fp3d_residual", "tomo_fp3d_residual_robust", "tomo_fp3d_residual_ring"]),
    "fused_epilogues": (ASYNC, ["tomo_bp3d_fista", "tomo_bp3d_fista_momentum", "tomo_bp3d_admm", "tomo_bp3d_matched_fista",
                                "tomo_bp3d_matched_fista_momentum", "tomo_bp3d_matched_admm"]),
    "volume_zquad": (ASYNC, ["tomo_volume_to_zquad", "tomo_momentum_transposed"]),
    "slicewise_tv": (ASYNC, ["tomo_pdtv_slices", "tomo_roftv_slices"]),
    "wavelets": (ASYNC, ["tomo_wavelet_shrink", "tomo_wavelet_forward", "tomo_wavelet_inverse"]),
    "patch_select_nltv": (ASYNC, ["tomo_patch_select", "tomo_nltv"]),
    "fbp_filter": (ASYNC, ["tomo_fbp_filter"]),
    "fourier_inv": (SYNC, ["tomo_fourier_inv"]),
    "elementwise": (ASYNC, ["tomo_momentum", "tomo_admm_dual", "tomo_axpby", "tomo_scale", "tomo_clamp_min", "tomo_mul",
                            "tomo_recip_safe", "tomo_fill", "tomo_pwls_weights_scaled"]),
    "pwls_weights": (SYNC, ["tomo_pwls_weights"]),      # it reduces the maximum to the host before it scales
    "reductions": (SYNC, ["tomo_norm2", "tomo_dot", "tomo_max", "tomo_pwls_max"]),
    "rel_change": (SYNC, ["tomo_rel_change"]),
    "pad_crop_mask_permute": (ASYNC, ["tomo_pad_edge", "tomo_crop_center", "tomo_circ_mask", "tomo_permute3"]),
    "sino_terms": (ASYNC, ["tomo_shift_rows", "tomo_sino_residual", "tomo_sino_add_ring", "tomo_sino_robust"]),
    "ring_terms": (ASYNC, ["tomo_ring_gh_reduce", "tomo_ring_gh_update", "tomo_swls_apply"]),
    "halo_staging": (ASYNC, ["tomo_halo_pack", "tomo_halo_unpack", "tomo_halo_pack2", "tomo_halo_pull2"]),
    "stream_kernels": (ASYNC, ["tomo_pdhg_sino_dual", "tomo_spdhg_sino_dual", "tomo_spdhg_primal"]),
    "diag_stream": (ASYNC, ["tomo_diag_stream"]),
    "pdtv": (ASYNC, ["tomo_pdtv"]),
    "roftv": (ASYNC, ["tomo_roftv"]),
    "pdtv_tol": (ASYNC, ["tomo_pdtv_tol"]),         # with tol 0; once more with tol > 0, values only
    "roftv_tol": (ASYNC, ["tomo_roftv_tol"]),
    "tgv": (ASYNC, ["tomo_tgv"]),
    "ndf": (ASYNC, ["tomo_ndf"]),
    "diff4th": (ASYNC, ["tomo_diff4th"]),
    "llt_rof": (ASYNC, ["tomo_llt_rof"]),
    "pdhg_marches": (ASYNC, ["tomo_pdhg_tv_dual", "tomo_pdhg_primal"]),
    "pdhg_diag": (ASYNC, ["tomo_pdhg_diag_steps", "tomo_pdhg_sino_dual_diag", "tomo_pdhg_primal_diag"]),
    "pdhg_tgv": (ASYNC, ["tomo_pdhg_tgv_dual", "tomo_pdhg_tgv_primal", "tomo_pdhg_tgv_primal_diag"]),
    "pdhg_stripe": (ASYNC, ["tomo_pdhg_sino_dual_stripe", "tomo_pdhg_stripe_update"]),
    "spdhg_tv": (ASYNC, ["tomo_spdhg_tv_dual", "tomo_spdhg_tv_primal"]),
    "reserve_scratch": (ASYNC, ["tomo_reserve_scratch"]),
    "placed_scratch": (ASYNC, ["tomo_placed_scratch"]),
    "pdtv_slabs": (ASYNC, ["tomo_pdtv_iter_slab", "tomo_pdtv_multi_slab_range"]),
    "roftv_slabs": (ASYNC, ["tomo_roftv_iter_slab_range"]),
    "march_slabs": (ASYNC, ["tomo_ndf_iter_slab_range", "tomo_diff4th_iter_slab_range", "tomo_llt_rof_iter_slab_range"]),
}

# entry point -> (case, kind)
TABLE = {name: (case, TOL if name in TOL_ENTRIES else kind) for case, (kind, names) in CASES.items() for name in names}
assert all(name in TABLE and TABLE[name][1] == TOL for name in TOL_ENTRIES)
assert len(TABLE) == sum(len(names) for _, names in CASES.values()), "an entry point is listed under two cases"
