"""graphminer_amd -- MI355X-native subgraph-matching hot path (TC / diamond / k-clique / 3-motif).

The product is the C-ABI shared library ``libgraphminer_amd.so`` (include/graphminer_amd.h,
hand-written HIP for gfx950). This package is the thin host-side mirror of the reference's
solver interface over that library; it contains no compute of its own and no CPU fallback.
"""
from ._lib import (GM_PART_RANGE, GM_PART_ROUND_ROBIN, GraphMinerBuildError, GraphMinerError, LIB_PATH, load)
from .graph import DeviceGraph, Graph, GraphFormatError
from .solvers import (SGL6_PATTERNS, SGL6_RAW, CliqueSolver, MotifSolver, SglSolver, Stats, TCSolver, clique_core_decompose, clique_kcore, clique_ktruss, clique_list, clique_local, clique_plan_info, clique_truss_decompose, ktruss, map_constants, map_plan_info, motif_local,
                      nucleus34, nucleus34_decompose, num_possible_patterns, rect_local, sgl6, sgl6_finish, sgl6_need, sgl6_raw, tc_list, tc_local,
                      tri_clique4_local, truss_decompose)

__all__ = [
    "Graph", "DeviceGraph", "GraphFormatError", "GraphMinerError", "GraphMinerBuildError",
    "TCSolver", "SglSolver", "CliqueSolver", "MotifSolver", "Stats", "num_possible_patterns",
    "tc_local", "ktruss", "truss_decompose", "tc_list", "clique_list", "clique_local", "clique_kcore", "clique_core_decompose", "clique_ktruss", "clique_truss_decompose", "tri_clique4_local", "nucleus34", "nucleus34_decompose", "rect_local", "motif_local", "map_constants", "map_plan_info", "clique_plan_info",
    "SGL6_PATTERNS", "SGL6_RAW", "sgl6", "sgl6_need", "sgl6_raw", "sgl6_finish",
    "GM_PART_ROUND_ROBIN", "GM_PART_RANGE", "LIB_PATH", "load",
]
