"""plinopt_amd -- MI355X (gfx950) drop-in for the hot path of jgdumas/plinopt:
the randomized multi-start search for minimum-cost straight-line programs.

Only what the path needs lives here: `csrc/` (HIP kernels + the C-ABI of
include/plinopt_hip.h, built into libplinopt_hip.so) and a thin host mirror of
the reference's restart-loop interface (search.py, dist.py)."""
from . import capi  # noqa: F401
from .search import CSEPlan, CSEPlanQ, cse_q_universe, CSEChain, TrilPlan, TRIL_BASE_SEED, cmp_op_count_key, cob_search, cob_search_batch, chain_batch, cse_batch_search, kernel_search, kernel_search_orders, kernel_batch_search, cse_search_multi, kernel_search_multi, tril_search_multi, LinPlan, LIN_BASE_SEED, lin_search_multi, OrbitPlan, ORBIT_BASE_SEED, ORBIT_DENSITY, ORBIT_CSE, ORBIT_CANONICAL, ORBIT_ACT_TRIANGULAR, ORBIT_ACT_PLUQ, ORBIT_ACT_HOUSEHOLDER, orbit_search_multi, ORBIT_GROWTH, OrbitGrowthPlan, orbit_growth_search_multi, DepPlan, DEP_ZERO, DEP_ONE, DEP_PRIME, BrentPlan, PolyMulPlan, TProgPlan  # noqa: F401
from .dist import shard_range, pack_key, allreduce_best, allreduce_tril_best  # noqa: F401
