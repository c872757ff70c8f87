"""
ctypes binding of the C-ABI library (include/pxmcmc_amd.h).  No torch types cross the
boundary: tensors are passed as raw device pointers + sizes, the stream as a void*.

The HIP library is the only compute path: if it is missing or fails to load this module
raises, it never falls back to a CPU implementation.
"""
import ctypes as C
import os

# torch first: it ships its own HIP runtime (torch/lib/libamdhip64.so).  If this library (linked against
# /opt/rocm's libamdhip64.so.7) were loaded before torch, the process would end up with two HIP runtimes and
# the second one sees no device.  With torch loaded first the loader resolves our dependency to the runtime
# torch already brought in, so kernels, streams and device pointers are shared.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PXM_LIB_PATH") or os.path.join(_HERE, "lib", "libpxmcmc_amd.so")  # override: A/B builds

c_i64, c_u64, c_int, c_dbl, c_vp = C.c_int64, C.c_uint64, C.c_int, C.c_double, C.c_void_p

# name -> (restype, argtypes): every symbol include/pxmcmc_amd.h declares
SIGNATURES = {
    "pxm_version": (c_int, []),
    "pxm_noise_bits": (c_int, []),
    "pxm_host_check_address_ranges": (c_i64, [c_int, c_dbl, c_int, c_int, c_int, c_int]),
    "pxm_host_gram_table_bytes": (c_i64, [c_int, c_dbl, c_int, c_int, c_int]),
    "pxm_last_error": (C.c_char_p, []),
    "pxm_device_count": (c_int, []),
    "pxm_capture_begin": (c_int, []),
    "pxm_capture_end": (c_int, []),
    "pxm_deferred_pending": (c_int, []),
    "pxm_tables_trim": (c_int, []),
    "pxm_wav_set_iter_counter": (c_int, [c_vp, c_vp]),
    "pxm_wav_release_iter_counter": (c_int, [c_vp, c_vp]),
    "pxm_wav_iter_counter_add": (c_int, [c_vp, c_u64, c_vp]),
    "pxm_wav_exact_dft_scales": (c_int, [c_vp]),
    "pxm_wav_dft_stock": (c_int, [c_vp]),
    "pxm_wav_mem_policy": (c_int, [c_vp]),
    "pxm_wav_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_sht_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_wav_profile_enable": (c_int, [c_vp, c_int]),
    "pxm_wav_profile_read": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pxm_wav_profile_read_launches": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "pxm_wav_profile_read_dft": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "pxm_wav_workspace_nonfinite": (c_i64, [c_vp, c_vp]),
    "pxm_wav_workspace_read": (c_i64, [c_vp, c_vp, c_i64, c_vp]),
    "pxm_reduce_scratch_doubles": (c_i64, [c_int]),
    "pxm_j_max": (c_int, [c_int, c_dbl]),
    "pxm_wav_bandlimits": (c_int, [c_int, c_dbl, c_int, c_vp, c_int]),
    "pxm_wav_ncoefs": (c_i64, [c_int, c_dbl, c_int, c_vp]),
    "pxm_tiling_axisym": (c_int, [c_int, c_dbl, c_int, c_vp, c_vp]),
    "pxm_mw_ring_weights": (c_int, [c_int, c_vp]),
    "pxm_host_sht_tables": (c_int, [c_int, c_int, c_int, c_vp, c_vp]),
    "pxm_host_rec_table": (c_int, [c_int, c_int, c_int, c_vp]),
    "pxm_host_rec_geometry": (c_int, [c_int, c_int, c_int, c_vp]),
    "pxm_host_pfa511_tables": (c_int, [c_vp, c_vp]),
    "pxm_host_dft_geometry": (c_int, [c_int, c_vp]),
    "pxm_host_dft_step_is_stock": (c_int, [C.c_uint, c_int, c_u64]),
    "pxm_quantile_range": (c_int, [c_vp, c_i64, c_i64, c_i64, c_dbl, c_vp, c_vp]),
    "pxm_moments_update": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_int, c_vp]),
    "pxm_moments_scratch_doubles": (c_i64, [c_i64]),
    "pxm_moments_finalize": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pxm_tails_buffer_doubles": (c_i64, [c_i64, c_int, c_i64]),
    "pxm_tails_stage_doubles": (c_i64, [c_i64, c_int]),
    "pxm_tails_update": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_i64, c_i64, c_vp]),
    "pxm_tails_quantiles": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_i64, c_i64, c_dbl, c_vp, c_vp, c_vp]),
    "pxm_acov_stage_depth": (c_int, []),
    "pxm_acov_state_doubles": (c_i64, [c_i64, c_int, c_int]),
    "pxm_acov_ring_doubles": (c_i64, [c_i64, c_int, c_int]),
    "pxm_acov_scratch_doubles": (c_i64, [c_i64]),
    "pxm_acov_update": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_acov_ess": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "pxm_sht_uses_recursion": (c_int, [c_vp]),
    "pxm_rec_reduce_selftest": (c_int, [c_vp]),
    "pxm_sht_plan_create": (c_int, [c_int, c_int, c_int, C.c_uint, C.POINTER(c_vp)]),
    "pxm_sht_plan_destroy": (c_int, [c_vp]),
    "pxm_sht_inverse": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_sht_forward": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_sht_inverse_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_sht_forward_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_sht_table_bytes": (c_i64, [c_vp, c_int]),
    "pxm_dft_plan_create": (c_int, [c_int, c_int, C.POINTER(c_vp)]),
    "pxm_dft_plan_destroy": (c_int, [c_vp]),
    "pxm_dft_px2ring": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dft_ring2px": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dft_px2ring_ex": (c_int, [c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_int, c_int, c_vp]),
    "pxm_dft_ring2px_ex": (c_int, [c_vp, c_vp, c_int, c_vp, c_i64, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_int, c_vp]),
    "pxm_dft_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_host_hpx_geometry": (c_int, [c_int, c_int, c_vp]),
    "pxm_host_hpx_rings": (c_int, [c_int, c_vp, c_vp, c_vp, c_vp]),
    "pxm_host_hpx_lambda": (c_int, [c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "pxm_hpx_plan_create": (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_vp)]),
    "pxm_hpx_plan_destroy": (c_int, [c_vp]),
    "pxm_hpx_synthesis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hpx_synthesis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hpx_table_bytes": (c_i64, [c_vp]),
    "pxm_hpx_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_gemm_plan_create": (c_int, [c_int, c_int, c_int, c_vp, c_int, C.POINTER(c_vp)]),
    "pxm_gemm_plan_destroy": (c_int, [c_vp]),
    "pxm_gemm_plan_report": (c_i64, [c_vp, c_int, c_int, c_vp, c_i64]),
    "pxm_host_gemm_plan_report": (c_i64, [c_int, c_int, c_int, c_vp, c_int, c_int, c_int, c_vp, c_i64]),
    "pxm_gemm_plan_write": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "pxm_gemm_plan_read": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "pxm_gemm_plan_table_read": (c_int, [c_vp, c_int, c_int, c_vp, c_i64, c_vp]),
    "pxm_gemm_plan_run": (c_int, [c_vp, c_int, c_int, c_dbl, c_dbl, c_dbl, c_int, c_vp]),
    "pxm_dwav_plan_create": (c_int, [c_int, c_dbl, c_int, c_int, c_int, C.c_uint, C.POINTER(c_vp)]),
    "pxm_dwav_plan_destroy": (c_int, [c_vp]),
    "pxm_dwav_synthesis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dwav_synthesis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dwav_analysis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dwav_analysis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_dwav_ncoefs": (c_i64, [c_int, c_dbl, c_int, c_int, c_vp]),
    "pxm_dwav_table_bytes": (c_i64, [c_vp]),
    "pxm_dwav_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_dwav_plan_info": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "pxm_dwav_workspace_layout": (c_i64, [c_vp, c_vp, c_i64]),
    "pxm_dwav_workspace_write": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "pxm_dwav_workspace_read": (c_int, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    "pxm_dwav_run_stage": (c_int, [c_vp, c_int, c_int, c_vp, c_int, c_vp]),
    "pxm_host_harm_weights": (c_i64, [c_int, c_dbl, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_i64]),
    "pxm_host_dir_component": (c_int, [c_int, c_int, c_vp]),
    "pxm_host_dwav_phases": (c_int, [c_int, c_vp]),
    "pxm_hwav_plan_create": (c_int, [c_int, c_dbl, c_int, c_int, c_int, c_int, C.c_uint, C.POINTER(c_vp)]),
    "pxm_hwav_plan_destroy": (c_int, [c_vp]),
    "pxm_hwav_synthesis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hwav_synthesis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hwav_analysis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hwav_analysis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_hwav_ncoefs": (c_i64, [c_int, c_dbl, c_int, c_int, c_vp]),
    "pxm_hwav_status": (c_int, [c_vp, c_int, c_vp]),
    "pxm_hwav_plan_info": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "pxm_hwav_myula_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_int, c_vp],
    ),
    "pxm_wav_plan_create": (c_int, [c_int, c_dbl, c_int, c_int, C.c_uint, C.POINTER(c_vp)]),
    "pxm_wav_plan_create_spin": (c_int, [c_int, c_dbl, c_int, c_int, c_int, C.c_uint, C.POINTER(c_vp)]),
    "pxm_wav_plan_destroy": (c_int, [c_vp]),
    "pxm_wav_synthesis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_synthesis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_analysis": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_analysis_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_table_bytes": (c_i64, [c_vp, c_int]),
    "pxm_wav_gradg_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_int, c_vp],
    ),
    "pxm_wav_image_init": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp]),
    "pxm_wav_image_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_int, c_vp],
    ),
    "pxm_wav_ring_set_data": (c_int, [c_vp, c_vp, c_vp]),
    "pxm_wav_ring_init": (c_int, [c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_ring_step": (
        c_int,
        [c_vp, c_vp, c_dbl, c_dbl, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_int, c_vp],
    ),
    "pxm_wav_ring_preds": (c_int, [c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_wl_attach": (c_int, [c_vp, c_vp, c_vp, c_i64]),
    "pxm_wav_wl_uses_recursion": (c_int, [c_vp]),
    "pxm_wav_wl_forward": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_wav_wl_adjoint": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp]),
    "pxm_soft": (c_int, [c_vp, c_vp, c_dbl, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_residual_grad": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_myula_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_dbl, c_vp, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_i64, c_int, c_int, c_vp],
    ),
    "pxm_chain_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_i64, c_int, c_int, c_vp],
    ),
    "pxm_skrock_stage": (
        c_int,
        [c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp,
         c_i64, c_int, c_int, c_vp],
    ),
    "pxm_fista_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_dbl, c_dbl, c_vp, c_i64, c_u64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int,
         c_vp],
    ),
    "pxm_fista_step_restart": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_dbl, c_dbl, c_vp, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_i64, c_int,
         c_int, c_vp],
    ),
    "pxm_pd_primal_step": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_pd_dual_step": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_cg_apply": (c_int, [c_vp, c_vp, c_vp, c_vp, c_dbl, c_i64, c_vp, c_vp, c_vp, c_dbl, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_cg_update": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_i64, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_gauss_prox": (c_int, [c_vp, c_vp, c_dbl, c_dbl, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_cg_rhs": (c_int, [c_vp, c_vp, c_dbl, c_vp, c_vp, c_dbl, c_i64, c_dbl, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_group_variance_draw": (
        c_int,
        [c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_dbl, c_dbl, c_dbl, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_i64,
         c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_int, c_vp],
    ),
    "pxm_lasso_precision_draw": (
        c_int,
        [c_vp, c_vp, c_dbl, c_dbl, c_vp, c_dbl, c_dbl, c_dbl, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int,
         c_vp],
    ),
    "pxm_tv_grad": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "pxm_tv_grad_adjoint": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "pxm_tv_value": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "pxm_pd_dual_step_pairs": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_tv_primal_step": (c_int, [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "pxm_tv_dual_step": (c_int, [c_vp, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp]),
    "pxm_lci_scratch_doubles": (c_i64, [c_i64, c_int]),
    "pxm_lci_data_terms": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_lci_eval": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_lci_search": (c_int, [c_vp, c_vp, c_vp, c_dbl, c_vp, c_dbl, c_vp, c_int, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_inpaint_scratch_doubles": (c_i64, [c_i64, c_int]),
    "pxm_inpaint_step": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_sapg_step": (
        c_int,
        [c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_dbl, c_vp, c_i64, c_dbl, c_dbl,
         c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_vp],
    ),
    "pxm_sapg_step_groups": (
        c_int,
        [c_vp, c_vp, c_vp, c_dbl, c_dbl, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_i64,
         c_dbl, c_dbl, c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_vp],
    ),
    "pxm_randn": (c_int, [c_vp, c_i64, c_int, c_int, c_u64, c_u64, c_u64, c_vp]),
    "pxm_box_muller": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_vp]),
    "pxm_reduce_l1": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_reduce_l2": (c_int, [c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_reduce_vdot": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_logtransition": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_dbl, c_dbl, c_vp, c_vp, c_i64, c_int, c_int, c_vp]),
    "pxm_pxmala_propose": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_dbl, c_vp, c_int, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
         c_i64, c_int, c_int, c_vp],
    ),
    "pxm_pxmala_accept": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_vp, c_vp, c_vp, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_int, c_dbl, c_vp, c_vp,
         c_int, c_int, c_vp],
    ),
    "pxm_pxmala_finish": (
        c_int,
        [c_vp, c_vp, c_vp, c_vp, c_dbl, c_vp, c_i64, c_int, c_vp, c_vp, c_vp, c_int, c_i64, c_int, c_vp, c_dbl, c_dbl, c_vp, c_vp,
         c_vp, c_vp, c_u64, c_u64, c_u64, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
         c_vp],
    ),
    "pxm_select_copy_many": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "pxm_counter_add": (c_int, [c_vp, c_u64, c_vp]),
    "pxm_wl_harmonic_mapping": (c_int, [c_vp, c_vp, c_vp, c_i64, c_int, c_vp]),
    "pxm_wl_mask_gather": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp]),
    "pxm_wl_mask_scatter": (c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, c_int, c_vp]),
    "pxm_csr_matvec": (c_int, [c_vp, c_vp, c_vp, c_int, c_i64, c_i64, c_vp, c_vp, c_int, c_int, c_vp, c_vp]),
}


class PxmError(RuntimeError):
    pass


# The integer ``#define PXM_<NAME>`` of include/pxmcmc_amd.h: each is mirrored once, here, as the module attribute <NAME>
# (tests/test_host_and_abi.py compares the block with the header in both directions).
CONSTANTS = dict(
    NOISE_F64=16,  # OR-ed into the mode / noise_complex / dtype argument of the noise-drawing entry points
    STATUS_PAIR_SYNC=2,  # bit of pxm_wav_status / pxm_sht_status (bit 0 is unused)
    MODE_REAL_NOISE=0,  # `mode` of the fused pxm_wav_*_step: real noise,
    MODE_CPLX_NOISE=1,  # complex noise,
    MODE_REAL_PAIRS=2,  # two real chains per complex slot
    FISTA_SLICES_MAX=256,  # partial sums per chain of pxm_fista_step
    CG_COEF=8,  # doubles per chain of the coefficient array of pxm_cg_apply / pxm_cg_update
    CG_FROZEN=1,  # bits of a chain's flags entry there
    CG_BREAKDOWN=2,
    GIBBS_SLICE=1024,  # elements per workgroup of pxm_group_variance_draw: the slice length of its table
    SAPG_SLICES_MAX=256,  # partial sums per chain of pxm_sapg_step (per chain and group of pxm_sapg_step_groups)
    SAPG_GROUPS_MAX=32,  # most groups of pxm_sapg_step_groups
    LCI_POINTS=32,  # values of xi per slot and pass of pxm_lci_eval
    LCI_ROUNDS_MAX=64,  # most passes of pxm_lci_search
    LCI_EMPTY=1,  # bits of the status of pxm_lci_search (0: ok)
    LCI_UNCONSTRAINED=2,
    LCI_NONFINITE=4,
    GEMM_SIDE_INTS=16,  # ints per side of pxm_gemm_plan_create
)
globals().update(CONSTANTS)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"pxmcmc_amd: HIP extension not built ({LIB_PATH} missing). "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C pxmcmc_amd/csrc`. "
            "There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc):
    """Raise if a C-ABI call returned an error code."""
    if rc is not None and rc < 0:
        raise PxmError(lib.pxm_last_error().decode())
    return rc


def require_gpu():
    if lib.pxm_device_count() < 1:
        raise PxmError("pxmcmc_amd: no HIP device visible; the HIP kernels are the only compute path")
