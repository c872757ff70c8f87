"""
Thin tensor-level wrappers over the C-ABI: torch supplies device memory and the stream,
every operation is a hand-written HIP kernel behind ``include/pxmcmc_amd.h``.

Conventions: arrays are ``[C, n]`` (chain batch first) or ``[n]`` (one chain); dtype is
float64 or complex128; outputs are fresh tensors (the reference never mutates inputs,
SURVEY.md section 8b).

One module per concern, as the kernel files are: ``steps`` (elementwise.hip, skrock.hip, fista.hip, primal_dual.hip, sapg.hip), ``reduce``
(reduce.hip), ``pxmala`` (pxmala.hip), ``summary`` (moments.hip, tails.hip, acov.hip), ``lci`` (lci.hip), ``inpaint`` (inpaint.hip),
``tv`` (tv.hip), ``cg`` (cg.hip), ``gibbs`` (gibbs.hip), ``lasso`` (lasso.hip), ``sparse`` (spmv.hip), ``plans`` (the plan sources), ``host`` (tables.cpp, host_api.cpp); ``_args`` holds what they do to their arguments
and the checks they share.  Callers use the names below as ``ops.<name>``.
"""
# flake8: noqa: F401  (every import below is a re-export)
from .._lib import (CG_BREAKDOWN, CG_COEF, CG_FROZEN, FISTA_SLICES_MAX, GIBBS_SLICE, LCI_EMPTY, LCI_NONFINITE, LCI_POINTS, LCI_UNCONSTRAINED, SAPG_GROUPS_MAX, SAPG_SLICES_MAX,
                    PxmError, check, require_gpu)
from ._args import GEMM_KINDS, _batched, _p, _stream, as_device, device
from .cg import cg_apply, cg_coef, cg_rhs, cg_scratch, cg_update, gauss_prox
from .gibbs import GibbsGroups, group_variance_draw
from .host import (DFT_STEP_FIELDS, DFT_UNITS, GEMM_TASK_FIELDS, dft_geometry, dft_step_is_stock, dir_component, dwav_phases, gemm_plan_geometry, gemm_report, harm_weights, hpx_geometry, hpx_lambda, hpx_rings, j_max, mw_ring_weights, noise_bits, rec_geometry, tiling_axisym,
                   wav_bandlimits)
from .inpaint import inpaint_scratch, inpaint_step
from .lasso import lasso_precision_draw, lasso_scratch
from .lci import lci_data_terms, lci_eval, lci_scratch, lci_search
from .plans import (DftPlan, DirWavPlan, GemmPlan, HarmWavPlan, HpxPlan, IterCounter, ShtPlan, WavPlan, _Plan, capture_scope, live_plans, raise_on_status,
                    tables_trim)
from .pxmala import logtransition, pxmala_accept, pxmala_finish, pxmala_propose, pxmala_propose_scratch
from .reduce import quantile_range, reduce_l1, reduce_l2, reduce_scratch_doubles, reduce_vdot
from .sparse import CsrMatrix
from .steps import (box_muller, chain_step, counter_add, fista_restart_scratch, fista_scratch, fista_step, fista_step_restart,
                    myula_step, pd_dual_step, pd_primal_step, pd_scratch, randn, residual_grad, sapg_group_bounds, sapg_groups_scratch, sapg_scratch, sapg_step,
                    sapg_step_groups, select_copy_many, skrock_stage, soft)
from .tv import pd_dual_step_pairs, tv_dual_step, tv_grad, tv_grad_adjoint, tv_primal_step, tv_ring_coefs, tv_value
from .summary import (acov_ess, acov_stage_depth, acov_update, moments_finalize, moments_update, tails_quantiles,
                      tails_stage_depth, tails_update)
