"""The numbers of include/lsdsort.h, each once (tests/test_python_face_cpu.py holds them to the header), and its status
codes as Python exceptions."""
from __future__ import annotations

LSDSORT_OK = 0
LSDSORT_ERR_INVALID_ARG = -1
LSDSORT_ERR_NO_DEVICE = -2
LSDSORT_ERR_HIP = -3
LSDSORT_ERR_WORKSPACE = -4
LSDSORT_ERR_TOO_LARGE = -5
LSDSORT_ERR_UNSUPPORTED = -6
LSDSORT_ERR_DEVICE_FAULT = -7
LSDSORT_ERR_COMM = -8
LSDSORT_ERR_CAPACITY = -9

LSDSORT_ALGO_ONESWEEP = 0
LSDSORT_ALGO_STAGED = 1

LSDSORT_MAX_KEYS = 0x3FFFFFFF
LSDSORT_MAX_PASSES = 32
LSDSORT_ROWS16_NATIVE_MAX_COLS = 262144   # lsdsort_rows16_device: longer rows take the widen route
LSDSORT_KTH_MAX_RANKS = 8                 # lsdsort_kth_multi_device: ranks per call
LSDSORT_LOGPROB_MAX_SLOTS = 32            # lsdsort_logprob16_device: ids per row and call

LSDSORT_KEY_U32, LSDSORT_KEY_I32, LSDSORT_KEY_F32 = 0, 1, 2
LSDSORT_KEY_U64, LSDSORT_KEY_I64, LSDSORT_KEY_F64 = 3, 4, 5
KEY_TYPES_32 = {"uint32": LSDSORT_KEY_U32, "int32": LSDSORT_KEY_I32, "float32": LSDSORT_KEY_F32}
KEY_TYPES_64 = {"uint64": LSDSORT_KEY_U64, "int64": LSDSORT_KEY_I64, "float64": LSDSORT_KEY_F64}
# lsdsort_key16_type: an enum of its own (lsdsort_keys16_device, lsdsort_topk16_device)
LSDSORT_KEY16_U16, LSDSORT_KEY16_I16, LSDSORT_KEY16_F16, LSDSORT_KEY16_BF16 = 0, 1, 2, 3
KEY_TYPES_16 = {"uint16": LSDSORT_KEY16_U16, "int16": LSDSORT_KEY16_I16, "float16": LSDSORT_KEY16_F16, "bfloat16": LSDSORT_KEY16_BF16}

# lsdsort_reduce_op and lsdsort_val_type (lsdsort_reduce_runs_device, lsdsort_reduce_by_key_device)
LSDSORT_REDUCE_SUM, LSDSORT_REDUCE_MIN, LSDSORT_REDUCE_MAX = 0, 1, 2
REDUCE_OPS = {"sum": LSDSORT_REDUCE_SUM, "min": LSDSORT_REDUCE_MIN, "max": LSDSORT_REDUCE_MAX}
LSDSORT_VAL_U32, LSDSORT_VAL_I32, LSDSORT_VAL_F32 = 0, 1, 2
VAL_TYPES = {"uint32": LSDSORT_VAL_U32, "int32": LSDSORT_VAL_I32, "float32": LSDSORT_VAL_F32}

LSDSORT_PARTITION_MSB = 0
LSDSORT_PARTITION_SPLITTERS = 1
PARTITIONS = {"msb": LSDSORT_PARTITION_MSB, "splitters": LSDSORT_PARTITION_SPLITTERS}


class LsdsortError(RuntimeError):
    """A C-ABI entry returned a negative status.  The reference crashes instead
    (MYCRASH, LSDRadixSort/Utils.h:6-15; CUDA_CALL, LSDRadixSort/CudaUtils.h:7-8)."""

    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: lsdsort status {status}: {detail}")


def check(status: int, where: str) -> None:
    if status != LSDSORT_OK:
        from ._lib import lib

        L = lib()
        detail = L.lsdsort_strerror(status).decode()
        if status == LSDSORT_ERR_HIP:
            detail += f" [{L.lsdsort_last_hip_error()}: {L.lsdsort_last_hip_error_string().decode()}]"
        if status == LSDSORT_ERR_COMM:
            detail += f" [{L.lsdsort_last_comm_error().decode()}]"
        raise LsdsortError(status, where, detail)
