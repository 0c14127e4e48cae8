"""lsdradixsort_amd -- MI355X-native (gfx950) LSD radix sort for uint32 keys and key/value pairs.

The product is ``liblsdsort.so`` (hand-written HIP kernels behind the C-ABI in
``include/lsdsort.h``); this package is its thin Python face for tests, ``bench.py`` and the
one-process-per-GPU driver (``dist.py``).  There is no CPU fallback: without the built
library, or without a gfx950 device, every entry raises.
"""
from .errors import (LSDSORT_ALGO_ONESWEEP, LSDSORT_ALGO_STAGED, LSDSORT_MAX_KEYS, LsdsortError)  # noqa: F401
from ._lib import LIB_PATH, lib  # noqa: F401
from .api import (  # noqa: F401  (api.__all__, name for name)
    sort, sort_pairs, to_device, to_host, workspace_bytes, alloc_workspace, workspace_form, workspace_half, tile_keys,
    set_tile_config, set_xcd_chunk, set_hybrid, set_half_hop, set_small_sort, set_pass_skipping, set_rank_method, rank_method,
    GPULSDRadixSort, GPULSDRadixSortTimed, GPUSortMulti, GPUSortTyped, GPUSortWide, sort64,
    GPUSort16, keys16_workspace_bytes, set_keys16_route, sort16, GPUTopK16, topk16_workspace_bytes, topk16_rows,
    GPUSortRows16, rows16_workspace_bytes, set_rows16_route, sort_rows16,
    GPUSortSegmented, segmented_workspace_bytes, sort_rows, GPUTopK, topk_workspace_bytes, topk_rows,
    GPUKth, kth_workspace_bytes, kthvalue_rows, median_rows,
    GPUKthMulti, kth_multi_workspace_bytes, quantile_rows, quantile_ranks,
    GPUKth16, kth16_workspace_bytes, kthvalue16_rows, median16_rows,
    GPUKth16Multi, kth16_multi_workspace_bytes, quantile16_rows,
    GPUKth16PerRow, kth16_perrow_workspace_bytes, GPUTopK16Filter, topk16_filter_workspace_bytes, topk16_filter_rows,
    GPUTopP16Filter, topp16_filter_workspace_bytes, topp16_filter_rows,
    GPUSample16, sample16_workspace_bytes, sample16_rows,
    GPULogprob16, logprob16_workspace_bytes, logprobs16_rows, top_logprobs16_rows,
    GPURunLength, GPUUnique, rle_workspace_bytes, unique_workspace_bytes, unique, unique_consecutive,
    GPUReduceRuns, GPUReduceByKey, reduce_runs_workspace_bytes, reduce_by_key_workspace_bytes, reduce_by_key, reduce_consecutive,
    BuildHistograms, BuildOffsets, RankScatter, DigitHistograms,
    MSBPartition, SplitterPartition, ThresholdPartition, sharded_thresholds,
)

__version__ = "0.1.0"
