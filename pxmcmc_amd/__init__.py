"""
pxmcmc_amd -- MI355X (gfx950) implementation of pxmcmc's proximal-Langevin hot path
(MYULA / PxMALA) behind the reference's ForwardOperator / Prior / PxMCMCParams plugin API.
All compute runs in hand-written HIP kernels reached through the C-ABI in
include/pxmcmc_amd.h; there is no CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    """``pxmcmc_amd.SAPG`` / ``pxmcmc_amd.sapg_rho_table``, imported on first use (importing the package itself loads
    nothing: the HIP library is loaded by the first module that needs it)"""
    if name in ("SAPG", "sapg_rho_table"):
        from . import sapg

        return getattr(sapg, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
