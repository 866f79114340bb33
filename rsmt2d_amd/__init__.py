"""rsmt2d_amd -- Python mirror of celestiaorg/rsmt2d's API over the MI355X engine.

The product is ``librsmt2d_hip.so`` (HIP kernels for gfx950 + C++ host runtime,
C ABI in ``include/rsmt2d_hip.h``).  This module is a thin ``ctypes`` binding
that keeps the reference's names and semantics so tests read like the
reference's own:

    codec = NewLeoRSCodec()                                   # leopard.go:101
    eds = ComputeExtendedDataSquare(shares, codec, NewDefaultTree)
    row_roots, col_roots = eds.RowRoots(), eds.ColRoots()
    eds2 = ImportExtendedDataSquare(flattened_with_nones, codec, NewDefaultTree)
    eds2.Repair(row_roots, col_roots)    # raises ErrByzantineData / ErrUnrepairableDataSquare

Every compute entry point runs the HIP path; with no GPU it raises
``DeviceError`` -- there is no CPU fallback.
"""
from __future__ import annotations

import base64
import ctypes
import json
import math
import os
import subprocess
import threading
from typing import Callable, List, Optional, Sequence

__all__ = [
    "Leopard", "Row", "Col", "Axis", "Codec", "LeoRSCodec", "NewLeoRSCodec",
    "ExtendedDataSquare", "ComputeExtendedDataSquare", "ImportExtendedDataSquare",
    "NewExtendedDataSquare", "NewDefaultTree", "Tree", "ErrByzantineData",
    "ComputeExtendedDataSquareWithBuffer", "BufferedTreeConstructor", "NmtParams",
    "ErasuredNamespacedMerkleTreeConstructor", "newErasuredNamespacedMerkleTreeConstructor",
    "TreePool", "newTreePool",
    "ErrUnrepairableDataSquare", "ErrUnevenChunks", "RSMError", "DeviceError",
    "library", "build", "device_context", "Proof", "Sample", "prove_samples_dev", "verify_samples_dev",
    "RSM_PROOF_OK", "RSM_PROOF_MALFORMED", "RSM_PROOF_ORDER", "RSM_PROOF_ROOT", "RSM_PROOF_OCCUPIED",
    "RSM_PROOF_NAMESPACE", "RSM_PROOF_INCOMPLETE", "verify_namespaces_dev", "verify_namespace_data",
    "RootRef", "RootProof", "data_roots_dev", "prove_roots_dev", "verify_samples_data_root_dev",
    "RepairResult", "repair_squares_dev", "scatter_samples_dev",
    "REPAIR_OK", "REPAIR_STUCK", "REPAIR_ENCODING", "REPAIR_ROOTS",
    "REPAIR_BYZANTINE", "BYZ_ROOT", "BYZ_ENCODING", "BYZ_TREE", "RepairCheck", "repair_squares_checked_dev",
    "gather_vectors_dev", "byzantine_data_dev",
    "FRAUD_VALID", "FRAUD_TOOFEW", "FRAUD_SHARE", "FRAUD_CONSISTENT", "FraudVerdict", "fraud_proof_samples",
    "verify_fraud_proofs_dev", "BadEncodingProof",
    "RangeQuery", "RangeProof", "ShareProof", "share_range_queries", "prove_ranges_dev", "verify_ranges_dev",
    "verify_ranges_data_root_dev",
    "RSM_COMMIT_ORDER", "RSM_COMMIT_TREE", "BlobRef", "SubTreeWidth", "MerkleMountainRangeSizes", "CreateCommitment",
    "blob_commitments_dev", "commitments_dev",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librsmt2d_hip.so")

Leopard = "Leopard"  # codecs.go:11
Row = 0              # extendeddatacrossword.go:15-18
Col = 1
Axis = int

# rsmt2d_hip.h return codes
RSM_OK, RSM_EINVAL, RSM_ESHARESIZE, RSM_ETOOFEW, RSM_ESHAPE, RSM_EDEVICE = 0, -1, -2, -3, -4, -5
RSM_ENOMEM, RSM_EUNSUPPORTED, RSM_EUNREPAIRABLE, RSM_EBYZANTINE, RSM_ECELL, RSM_ETREE = -6, -7, -8, -9, -10, -11
# proof verification status words (one per sample; the first condition that applies wins)
RSM_PROOF_OK, RSM_PROOF_MALFORMED, RSM_PROOF_ORDER, RSM_PROOF_ROOT, RSM_PROOF_OCCUPIED = 0, 1, 2, 3, 4
# namespace proofs only: a share of another namespace / shares of the namespace left out
RSM_PROOF_NAMESPACE, RSM_PROOF_INCOMPLETE = 5, 6
# share commitment status words (one per blob)
RSM_COMMIT_ORDER, RSM_COMMIT_TREE = 1, 2


class RSMError(Exception):
    """Error returned by the C ABI (code = RSM_E*)."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class DeviceError(RSMError):
    """No usable GPU / HIP failure.  The product never falls back to the CPU."""


class _Unrepairable(RSMError):
    pass


#: ErrUnrepairableDataSquare (extendeddatacrossword.go:37) -- a singleton like the Go sentinel.
ErrUnrepairableDataSquare = _Unrepairable(RSM_EUNREPAIRABLE, "failed to solve data square")

#: ErrUnevenChunks (datasquare.go:14)
ErrUnevenChunks = "non-nil shares not all of equal size"


class ErrByzantineData(RSMError):
    """ErrByzantineData (extendeddatacrossword.go:42-58): Axis, Index, Shares (None = missing)."""

    def __init__(self, axis: int, index: int, shares: List[Optional[bytes]]):
        super().__init__(RSM_EBYZANTINE, f"byzantine {'row' if axis == Row else 'col'}: {index}")
        self.Axis = axis
        self.Index = index
        self.Shares = shares


# ---------------------------------------------------------------------------
# library loading
# ---------------------------------------------------------------------------
_lib = None
# re-entrant: a __del__ run by the garbage collector while the lock is held calls library()
_lib_lock = threading.RLock()
_TREE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                            ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32,
                            ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32))


class _Byz(ctypes.Structure):
    _fields_ = [("axis", ctypes.c_int32), ("index", ctypes.c_uint32)]


class NmtParams(ctypes.Structure):
    """rsm_nmt_params (include/rsmt2d_hip.h)."""
    _fields_ = [("namespace_size", ctypes.c_uint32), ("ignore_max_namespace", ctypes.c_uint32),
                ("square_size", ctypes.c_uint32)]


#: rsm_repair_stats.fallback_reason: which step sent the last Repair from the device
#: fast path to the exact sequential solver (include/rsmt2d_hip.h)
FALLBACK_NONE, FALLBACK_STUCK, FALLBACK_ENCODING, FALLBACK_ROOTS = 0, 1, 2, 3


class RepairStats(ctypes.Structure):
    """rsm_repair_stats (include/rsmt2d_hip.h): counters of the last Repair."""
    _fields_ =[("fast_path", ctypes.c_int32), ("sweeps", ctypes.c_uint32),
                ("decoded_vectors", ctypes.c_uint32), ("fallback_reason", ctypes.c_uint32)]


#: rsm_repair_result.status of rsm_repair_squares_dev (include/rsmt2d_hip.h)
REPAIR_OK, REPAIR_STUCK, REPAIR_ENCODING, REPAIR_ROOTS = 0, 1, 2, 3


class RepairResult(ctypes.Structure):
    """rsm_repair_result (include/rsmt2d_hip.h): one square of rsm_repair_squares_dev."""
    _fields_ = [("status", ctypes.c_uint32), ("sweeps", ctypes.c_uint32),
                ("decoded_vectors", ctypes.c_uint32), ("missing", ctypes.c_uint32)]


#: rsm_repair_squares_checked_dev: the status of a square with a bad vector, and
#: rsm_repair_check.reason
REPAIR_BYZANTINE = 4
BYZ_ROOT, BYZ_ENCODING, BYZ_TREE = 1, 2, 3


class RepairCheck(ctypes.Structure):
    """rsm_repair_check (include/rsmt2d_hip.h): one square of rsm_repair_squares_checked_dev."""
    _fields_ = [("axis", ctypes.c_uint32), ("index", ctypes.c_uint32), ("round", ctypes.c_uint32),
                ("reason", ctypes.c_uint32), ("checked_vectors", ctypes.c_uint32), ("hashed_cells", ctypes.c_uint32)]


#: rsm_fraud_verdict.verdict of rsm_fraud_proofs_verify_dev (include/rsmt2d_hip.h)
FRAUD_VALID, FRAUD_TOOFEW, FRAUD_SHARE, FRAUD_CONSISTENT = 0, 1, 2, 3


class FraudVerdict(ctypes.Structure):
    """rsm_fraud_verdict (include/rsmt2d_hip.h): one proof of rsm_fraud_proofs_verify_dev.
    ``reason``: BYZ_* of a FRAUD_VALID proof, the RSM_PROOF_* word of slot ``pos`` of a
    FRAUD_SHARE one; ``present``: the non-zero presence bytes."""
    _fields_ = [("verdict", ctypes.c_uint32), ("reason", ctypes.c_uint32), ("pos", ctypes.c_uint32),
                ("present", ctypes.c_uint32)]


# (name, restype, argtypes) of every symbol declared in include/rsmt2d_hip.h
_VP, _U8P, _U32, _I32, _I64, _U64 = (ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                     ctypes.c_int, ctypes.c_int64, ctypes.c_uint64)
SIGNATURES = {
    "rsm_ctx_create": (_I32, [_I32, ctypes.POINTER(_VP)]),
    "rsm_ctx_destroy": (None, [_VP]),
    "rsm_ctx_device": (_I32, [_VP]),
    "rsm_ctx_set_pass_grid": (_I32, [_VP, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "rsm_ctx_set_split_max": (_I32, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "rsm_ctx_set_limits": (_I32, [_VP, _U64, _U64]),
    "rsm_last_error": (ctypes.c_char_p, []),
    "rsm_version": (ctypes.c_char_p, []),
    "rsm_device_count": (_I32, []),
    "rsm_codec_name": (ctypes.c_char_p, []),
    "rsm_codec_max_chunks": (_I64, []),
    "rsm_codec_validate_chunk_size": (_I32, [_I64]),
    "rsm_codec_field_bits": (_I32, [_U32]),
    "rsm_encode": (_I32, [_VP, _VP, _U32, _U32, _VP]),
    "rsm_decode": (_I32, [_VP, _VP, _VP, _U32, _U32]),
    "rsm_extend_square": (_I32, [_VP, _VP, _U32, _U32, _VP]),
    "rsm_extend_square_inplace_host": (_I32, [_VP, _VP, _U32, _U32]),
    "rsm_extend_squares_host": (_I32, [_VP, _VP, _U32, _U32, _U32, _VP]),
    "rsm_host_alloc": (_I32, [_VP, _U64, ctypes.POINTER(_VP)]),
    "rsm_host_free": (_I32, [_VP, _VP]),
    "rsm_multi_create": (_I32, [_VP, ctypes.c_int, ctypes.POINTER(_VP)]),
    "rsm_multi_destroy": (None, [_VP]),
    "rsm_multi_size": (_I32, [_VP]),
    "rsm_multi_context": (_VP, [_VP, ctypes.c_int]),
    "rsm_multi_extend_square": (_I32, [_VP, _VP, _U32, _U32, _VP, ctypes.c_int]),
    "rsm_multi_extend_dev": (_I32, [_VP, _VP, _U32, _U32, ctypes.c_int]),
    "rsm_multi_sync": (_I32, [_VP]),
    "rsm_multi_host_alloc": (_I32, [_VP, _U64, ctypes.POINTER(_VP)]),
    "rsm_multi_host_free": (_I32, [_VP, _VP]),
    "rsm_multi_extend_square_inplace": (_I32, [_VP, _VP, _U32, _U32, ctypes.c_int]),
    "rsm_extend_squares_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _VP]),
    "rsm_extend_squares_phase_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _I32, _VP]),
    "rsm_extend_rows_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _U32, _VP]),
    "rsm_extend_rows_blocks_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _U32, _VP, _U32, _VP]),
    "rsm_extend_cols_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _U32, _VP]),
    "rsm_roots_dev": (_I32, [_VP, _VP, _U32, _U32, _VP, _VP]),
    "rsm_roots_squares_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _VP, _VP]),
    "rsm_encode_batch_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, _U64, _U64, _VP]),
    "rsm_decode_vectors_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _I32, _VP, _U32, _VP]),
    "rsm_ctx_stream": (_VP, [_VP]),
    "rsm_dev_alloc": (_I32, [_VP, _U64, ctypes.POINTER(_VP)]),
    "rsm_dev_free": (_I32, [_VP, _VP]),
    "rsm_memcpy": (_I32, [_VP, _VP, _VP, _U64, _I32]),
    "rsm_dev_fill_random": (_I32, [_VP, _VP, _U64, _U64]),
    "rsm_sync": (_I32, [_VP]),
    "rsm_event_create": (_I32, [_VP, ctypes.POINTER(_VP)]),
    "rsm_event_destroy": (_I32, [_VP]),
    "rsm_event_record": (_I32, [_VP, _VP, _VP]),
    "rsm_event_elapsed_ms": (_I32, [_VP, _VP, ctypes.POINTER(ctypes.c_float)]),
    "rsm_stream_create": (_I32, [_VP, ctypes.POINTER(_VP)]),
    "rsm_stream_destroy": (_I32, [_VP, _VP]),
    "rsm_stream_sync": (_I32, [_VP]),
    "rsm_stream_check": (_I32, [_VP, _VP]),
    "rsm_dev_equal": (_I32, [_VP, _VP, _VP, _U64, _VP, ctypes.POINTER(ctypes.c_int)]),
    "rsm_time_extend": (_I32, [_VP, _VP, _U32, _U32, _U32, _U32, ctypes.POINTER(ctypes.c_float),
                               ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "rsm_default_tree_root": (_I32, [_VP, _I32, _U32, _VP, _U32, _U32, _VP, _VP]),
    "rsm_nmt_tree_root": (_I32, [_VP, _I32, _U32, _VP, _U32, _U32, _VP, _VP]),
    "rsm_nmt_roots_dev": (_I32, [_VP, _VP, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP, _VP]),
    "rsm_nmt_roots_squares_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP, _VP]),
    "rsm_eds_compute": (_I32, [_VP, _VP, _VP, _U64, ctypes.POINTER(_VP)]),
    "rsm_eds_import": (_I32, [_VP, _VP, _VP, _U64, ctypes.POINTER(_VP)]),
    "rsm_eds_new": (_I32, [_VP, _U32, _U32, ctypes.POINTER(_VP)]),
    "rsm_eds_free": (None, [_VP]),
    "rsm_eds_set_context": (_I32, [_VP, _VP]),
    "rsm_eds_width": (_U32, [_VP]),
    "rsm_eds_original_width": (_U32, [_VP]),
    "rsm_eds_share_size": (_U32, [_VP]),
    "rsm_eds_get_cell": (_I32, [_VP, _U32, _U32, _VP]),
    "rsm_eds_set_cell": (_I32, [_VP, _U32, _U32, _VP, _U32]),
    "rsm_eds_overwrite_cell": (_I32, [_VP, _U32, _U32, _VP, _U32]),
    "rsm_eds_flattened": (_I32, [_VP, _VP, _VP]),
    "rsm_eds_roots": (_I32, [_VP, _I32, _VP, _VP, _VP, _U32, ctypes.POINTER(_U32)]),
    "rsm_eds_repair": (_I32, [_VP, _VP, _VP, _U32, _VP, _VP, ctypes.POINTER(_Byz)]),
    "rsm_eds_byzantine_shares": (_I32, [_VP, _VP, _VP]),
    "rsm_eds_repair_stats": (_I32, [_VP, ctypes.POINTER(RepairStats)]),
    "rsm_proof_nodes_bytes": (_U64, [_U32, ctypes.POINTER(NmtParams), _U32]),
    "rsm_proof_record_bytes": (_U32, [_U32, ctypes.POINTER(NmtParams)]),
    "rsm_proof_nodes_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP, _VP, _VP]),
    "rsm_proofs_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _U32, _VP, _VP, _VP]),
    "rsm_default_tree_prove": (_I32, [_VP, _U32, _U32, _U32, _VP, _VP]),
    "rsm_nmt_tree_prove": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _U32, _U32, _U32, _VP, _VP]),
    "rsm_eds_proofs": (_I32, [_VP, _VP, _VP, _VP, _U32, _VP, _VP]),
    "rsm_proofs_verify_dev": (_I32, [_VP, _VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _U32, _VP, _VP]),
    "rsm_default_tree_verify": (_I32, [_VP, _U32, _U32, _U32, _VP, _VP, ctypes.POINTER(_U32)]),
    "rsm_nmt_tree_verify": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _U32, _U32, _U32, _VP, _VP,
                                   ctypes.POINTER(_U32)]),
    "rsm_ns_record_bytes": (_U32, [_U32, ctypes.POINTER(NmtParams)]),
    "rsm_ns_proofs_dev": (_I32, [_VP, _VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP, _U32, _VP, _VP,
                                 _VP, _U64, _VP]),
    "rsm_nmt_namespace_prove": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _U32, _U32, _VP, _VP, _VP]),
    "rsm_nmt_namespace_verify": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _VP, _U32, _U32, _U32, _VP, _VP,
                                        ctypes.POINTER(_U32)]),
    "rsm_ns_proofs_verify_dev": (_I32, [_VP, _VP, _VP, _VP, _U64, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP,
                                        _U32, _VP, _VP]),
    "rsm_range_record_bytes": (_U32, [_U32, ctypes.POINTER(NmtParams)]),
    "rsm_range_proofs_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _U32, _VP, _VP, _VP, _U64,
                                    _VP]),
    "rsm_default_tree_range_prove": (_I32, [_VP, _U32, _U32, _U32, _U32, _VP, _VP]),
    "rsm_nmt_tree_range_prove": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _U32, _U32, _U32, _U32, _VP, _VP]),
    "rsm_default_tree_range_verify": (_I32, [_U32, _U32, _VP, _U32, _U32, _U32, _VP, _VP, ctypes.POINTER(_U32)]),
    "rsm_nmt_tree_range_verify": (_I32, [ctypes.POINTER(NmtParams), _U32, _U32, _U32, _VP, _U32, _U32, _U32, _VP, _VP,
                                         ctypes.POINTER(_U32)]),
    "rsm_range_proofs_verify_dev": (_I32, [_VP, _VP, _VP, _VP, _U64, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP,
                                           _U32, _VP, _VP]),
    "rsm_range_proofs_verify_data_root_dev": (_I32, [_VP, _VP, _VP, _VP, _U64, _VP, _VP, _U32, _U32, _U32,
                                                     ctypes.POINTER(NmtParams), _VP, _U32, _VP, _VP]),
    "rsm_share_range_queries": (_I32, [_U32, _U32, _U32, _U32, _VP, ctypes.POINTER(_U32)]),
    "rsm_eds_range_proofs": (_I32, [_VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _U64]),
    "rsm_subtree_width": (_U32, [_U32, _U32]),
    "rsm_subtree_sizes": (_I32, [_U32, _U32, _VP, _U32, ctypes.POINTER(_U32)]),
    "rsm_blob_commitment": (_I32, [ctypes.POINTER(NmtParams), _VP, _U32, _U32, _U32, _VP, ctypes.POINTER(_U32)]),
    "rsm_square_commitment": (_I32, [ctypes.POINTER(NmtParams), _VP, _VP, _U32, _U32, _U32, _U32, _U32, _VP, _VP,
                                     ctypes.POINTER(_U32)]),
    "rsm_commit_work_bytes": (_U64, [_U64, _U64, ctypes.POINTER(NmtParams)]),
    "rsm_blob_commitments_dev": (_I32, [_VP, _VP, _U32, ctypes.POINTER(NmtParams), _U32, _VP, _U32, _VP, _VP, _VP, _VP]),
    "rsm_commitments_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, ctypes.POINTER(NmtParams), _U32, _VP, _U32, _VP, _VP, _VP, _VP,
                                   _VP]),
    "rsm_eds_commitments": (_I32, [_VP, _VP, _VP, _VP, _U32, _U32, _VP, _VP]),
    "rsm_eds_subtree_roots": (_I32, [_VP, _VP, _VP, _VP, _U32, _U32, _VP, _VP, _VP, _VP]),
    "rsm_eds_namespace_proofs": (_I32, [_VP, _VP, _VP, _I32, _VP, _U32, _VP, _VP, _VP, _VP, _U64]),
    "rsm_eds_import_samples": (_I32, [_VP, _VP, _VP, _U32, _VP, _VP, _VP, _U32, _VP, _VP, _VP, ctypes.POINTER(_U32)]),
    "rsm_data_root_record_bytes": (_U32, [_U32]),
    "rsm_data_root_nodes_bytes": (_U64, [_U32, _U32]),
    "rsm_data_roots_dev": (_I32, [_VP, _VP, _U32, _U32, _U32, _VP, _VP, _VP]),
    "rsm_root_proofs_dev": (_I32, [_VP, _VP, _U32, _U32, _VP, _U32, _VP, _VP]),
    "rsm_proofs_verify_data_root_dev": (_I32, [_VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP,
                                               _U32, _VP, _VP]),
    "rsm_data_root": (_I32, [_VP, _U32, _U32, _VP]),
    "rsm_data_root_prove": (_I32, [_VP, _U32, _U32, _U32, _U32, _VP]),
    "rsm_data_root_verify": (_I32, [_VP, _U32, _U32, _U32, _U32, _VP, _VP, ctypes.POINTER(_U32)]),
    "rsm_sample_verify_data_root": (_I32, [ctypes.POINTER(NmtParams), _U32, _VP, _VP, _U32, _VP, _VP, _VP,
                                           ctypes.POINTER(_U32)]),
    "rsm_eds_data_root": (_I32, [_VP, _VP, _VP, _VP]),
    "rsm_repair_work_bytes": (_U64, [_U32, _U32, _U32, ctypes.POINTER(NmtParams)]),
    "rsm_repair_squares_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP,
                                      ctypes.POINTER(RepairResult), _VP]),
    "rsm_repair_checked_work_bytes": (_U64, [_U32, _U32, _U32, ctypes.POINTER(NmtParams)]),
    "rsm_repair_squares_checked_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _VP,
                                              ctypes.POINTER(RepairResult), ctypes.POINTER(RepairCheck), _VP]),
    "rsm_vectors_gather_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, _VP, _U32, _VP, _VP, _VP]),
    "rsm_samples_scatter_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, _VP, _U32, _VP, _VP, _VP]),
    "rsm_fraud_work_bytes": (_U64, [_U32, _U32, _U32, ctypes.POINTER(NmtParams)]),
    "rsm_fraud_proof_samples": (_I32, [_VP, _U32, _VP]),
    "rsm_fraud_proofs_verify_dev": (_I32, [_VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, ctypes.POINTER(NmtParams), _VP, _U32,
                                           _VP, ctypes.POINTER(FraudVerdict), _VP]),
}


#: entry points of the diagnostic library only (include/rsmt2d_hip_diag.h)
DIAG_SIGNATURES = {
    "rsm_diag_set_bs_mode": (_I32, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rsm_diag_set_trace": (_I32, [_VP]),
    "rsm_diag_set_dec_trace": (_I32, [_VP]),
    "rsm_diag_set_split_waves": (_I32, [ctypes.c_int, ctypes.c_int]),
    "rsm_diag_set_split_fused": (_I32, [ctypes.c_int]),
    "rsm_diag_set_dec_delay": (_I32, [ctypes.c_uint32]),
    "rsm_diag_set_dec8_mode": (_I32, [ctypes.c_uint32]),
    "rsm_diag_set_codec_spin": (_I32, [ctypes.c_uint32]),
    "rsm_diag_set_repair_mode": (_I32, [ctypes.c_uint32]),
    "rsm_diag_set_dec16_mode": (_I32, [ctypes.c_uint32]),
    "rsm_diag_set_bs_row_mode": (_I32, [ctypes.c_int]),
    "rsm_diag_extend_fused": (_I32, [_VP, _VP, _U32, _U32, _U32, _U32, _VP]),
    "rsm_diag_queue_check": (_I32, [_VP, _VP]),
    "rsm_diag_extend_pipeline_dev": (_I32, [_VP, _VP, _VP, _U32, _U32, _U32, _VP]),
    "rsm_diag_alltoall_emulated": (_I32, [_VP, _VP, ctypes.c_int, _U32, _U32]),
}
# (A/B runs may point the DIAGNOSTIC library at a variant build; the product library
# path is fixed)
DIAG_LIB_PATH = os.environ.get("RSM_DIAG_LIB") or os.path.join(_HERE, "librsmt2d_hip_diag.so")


def build(diag: bool = True) -> str:
    """Compile librsmt2d_hip.so for gfx950 (make in rsmt2d_amd/csrc); with ``diag``
    also the measurement-only librsmt2d_hip_diag.so (-DRSM_DIAG)."""
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")], check=True)
    if diag:
        subprocess.run(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc"), "diag"], check=True)
    return LIB_PATH


_diag = None


def diag_library() -> ctypes.CDLL:
    """The DIAGNOSTIC library (A-B / no-arithmetic / fused kernels): measurement
    tooling, never the product.  It carries its own HIP state: do not mix its
    contexts with library()'s."""
    global _diag
    with _lib_lock:
        if _diag is None:
            if not os.path.exists(DIAG_LIB_PATH):
                raise DeviceError(RSM_EDEVICE, f"{DIAG_LIB_PATH} is missing: run rsmt2d_amd.build()")
            L = ctypes.CDLL(DIAG_LIB_PATH)
            for name, (res, args) in list(SIGNATURES.items()) + list(DIAG_SIGNATURES.items()):
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            _diag = L
    return _diag


def library() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise DeviceError(RSM_EDEVICE, f"{LIB_PATH} is missing: run rsmt2d_amd.build() "
                                               "(the HIP extension is required; there is no CPU path)")
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
            _lib = L
    return _lib


def _err(rc: int) -> RSMError:
    msg = (library().rsm_last_error() or b"").decode(errors="replace")
    if rc == RSM_EDEVICE:
        return DeviceError(rc, msg)
    return RSMError(rc, msg)


def _check(rc: int) -> None:
    if rc != RSM_OK:
        raise _err(rc)


def _check_with(L: ctypes.CDLL, rc: int) -> None:
    """_check for a call into another copy of the ABI (the diagnostic library)."""
    if rc != RSM_OK:
        msg = (L.rsm_last_error() or b"").decode(errors="replace")
        raise (DeviceError if rc == RSM_EDEVICE else RSMError)(rc, msg)


_ctx = {}
_ctx_lock = threading.Lock()


def device_context(device: int = 0) -> int:
    """The per-process rsm_ctx for a GPU (created on first use)."""
    with _ctx_lock:
        if device not in _ctx:
            h = ctypes.c_void_p()
            _check(library().rsm_ctx_create(device, ctypes.byref(h)))
            _ctx[device] = h.value
        return _ctx[device]


class DeviceBuffer:
    """Device memory owned by this library's HIP runtime (bench / tests plumbing)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.ctx = device_context(device)
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        _check(library().rsm_dev_alloc(self.ctx, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def fill_random(self, seed: int):
        _check(library().rsm_dev_fill_random(self.ctx, self.ptr, self.nbytes, seed))

    def upload(self, arr, offset: int = 0):
        import numpy as np
        a = np.ascontiguousarray(arr)
        _check(library().rsm_memcpy(self.ctx, self.ptr + offset, a.ctypes.data, a.nbytes, 0))

    def download(self, nbytes: int = None, offset: int = 0):
        import numpy as np
        n = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(n, np.uint8)
        _check(library().rsm_memcpy(self.ctx, out.ctypes.data, self.ptr + offset, n, 1))
        return out

    def free(self):
        if self.ptr:
            library().rsm_dev_free(self.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _bufs(shares: Sequence[Optional[bytes]]):
    """Keeps the bytes objects alive; returns (keepalive, void* array, u32 lens)."""
    n = len(shares)
    ptrs = (ctypes.c_void_p * max(n, 1))()
    lens = (ctypes.c_uint32 * max(n, 1))()
    keep = []
    for i, s in enumerate(shares):
        if s is None:
            ptrs[i] = None
            lens[i] = 0
        else:
            b = ctypes.create_string_buffer(bytes(s), len(s))
            keep.append(b)
            ptrs[i] = ctypes.cast(b, ctypes.c_void_p)
            lens[i] = len(s)
    return keep, ptrs, lens


# ---------------------------------------------------------------------------
# Codec (codecs.go:14-30) and LeoRSCodec (leopard.go)
# ---------------------------------------------------------------------------
class Codec:
    def Encode(self, data):  # pragma: no cover - interface
        raise NotImplementedError

    def Decode(self, data):  # pragma: no cover - interface
        raise NotImplementedError

    def MaxChunks(self) -> int:  # pragma: no cover - interface
        raise NotImplementedError

    def Name(self) -> str:  # pragma: no cover - interface
        raise NotImplementedError

    def ValidateChunkSize(self, chunkSize: int):  # pragma: no cover - interface
        raise NotImplementedError


class LeoRSCodec(Codec):
    """HIP-backed drop-in for rsmt2d.LeoRSCodec (leopard.go:16-103)."""

    def __init__(self, device: int = 0):
        self.device = device

    def Encode(self, data: Sequence[bytes]) -> List[bytes]:
        k = len(data)
        if k == 0:
            raise RSMError(RSM_EINVAL, "no shares")
        S = len(data[0])
        if any(d is None or len(d) != S for d in data):
            raise RSMError(RSM_ESHAPE, "shard sizes do not match")
        keep, ptrs, _ = _bufs(data)
        outs = [ctypes.create_string_buffer(S) for _ in range(k)]
        optr = (ctypes.c_void_p * k)(*[ctypes.cast(o, ctypes.c_void_p) for o in outs])
        _check(library().rsm_encode(device_context(self.device), ptrs, k, S, optr))
        return [o.raw for o in outs]

    def Decode(self, data: List[Optional[bytes]]) -> List[Optional[bytes]]:
        """Fills the None entries of ``data`` in place (as klauspost Reconstruct does)
        and returns the same list; raises RSMError(RSM_ETOOFEW) if < half present."""
        n = len(data)
        S = next((len(d) for d in data if d is not None), 0)
        present = (ctypes.c_uint8 * n)(*[0 if d is None else 1 for d in data])
        bufs = [ctypes.create_string_buffer(bytes(d) if d is not None else S, S) for d in data]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) for b in bufs])
        _check(library().rsm_decode(device_context(self.device), ptrs, present, n, S))
        for i in range(n):
            if data[i] is None:
                data[i] = bufs[i].raw
        return data

    def MaxChunks(self) -> int:
        return int(library().rsm_codec_max_chunks())

    def Name(self) -> str:
        return library().rsm_codec_name().decode()

    def ValidateChunkSize(self, chunkSize: int):
        rc = library().rsm_codec_validate_chunk_size(int(chunkSize))
        if rc != RSM_OK:
            return _err(rc)
        return None


def NewLeoRSCodec(device: int = 0) -> LeoRSCodec:
    return LeoRSCodec(device)


# codecs registry (codecs.go:32-40), used by JSON unmarshalling
codecs = {Leopard: NewLeoRSCodec()}


# ---------------------------------------------------------------------------
# Tree plugin (tree.go)
# ---------------------------------------------------------------------------
class Tree:
    """Tree interface: Push(data) / Root() -> bytes."""

    def Push(self, data: bytes):  # pragma: no cover - interface
        raise NotImplementedError

    def Root(self) -> bytes:  # pragma: no cover - interface
        raise NotImplementedError


def NewDefaultTree(axis: int = Row, index: int = 0):
    """Marker for the built-in DefaultTree (SHA-256 merkletree, tree.go:38)."""
    return None


class _NmtTree(Tree):
    """Host Tree of the erasured NMT (Push validates and collects, Root hashes via
    rsm_nmt_tree_root).  Push reports the wrapper's errors where the reference does
    (nmtwrapper_test.go:103-108: share or axis index past 2*squareSize, data shorter
    than the namespace) and the NMT's namespace push-order error (celestiaorg/nmt
    v0.24.3 Push: namespaces must not decrease; the parity namespace 0xFF.. is the
    largest)."""

    def __init__(self, params: "NmtParams", axis: int, index: int):
        self._p, self._axis, self._index, self._leaves = params, axis, index, []
        self._last_ns = None

    def Push(self, data: bytes):
        ns, n = self._p.namespace_size, int(self._p.square_size)
        share = len(self._leaves)
        if self._index + 1 > 2 * n or share + 1 > 2 * n:
            raise RSMError(RSM_EINVAL, f"pushed past predetermined square size: boundary at {2 * n} index at "
                                       f"{self._index} {share}")
        data = bytes(data)
        if len(data) < ns:
            raise RSMError(RSM_EINVAL, "data is too short to contain namespace ID")
        nid = data[:ns] if (share < n and self._index < n) else b"\xff" * ns
        if self._last_ns is not None and nid < self._last_ns:
            raise RSMError(RSM_EINVAL, "pushed data has to be lexicographically ordered by namespace IDs")
        self._last_ns = nid
        self._leaves.append(data)

    def Root(self) -> bytes:
        keep, ptrs, _ = _bufs(self._leaves) if self._leaves else ([], None, None)
        cap = 2 * self._p.namespace_size + 32
        out = (ctypes.c_uint8 * cap)()
        ln = ctypes.c_uint32(cap)
        size = len(self._leaves[0]) if self._leaves else 0
        if any(len(x) != size for x in self._leaves):
            raise ValueError("NMT leaves of unequal size")
        rc = library().rsm_nmt_tree_root(ctypes.byref(self._p), self._axis, self._index, ptrs, len(self._leaves),
                                         size, out, ctypes.byref(ln))
        if rc:
            raise _err(rc)
        return bytes(out[:ln.value])


class ErasuredNamespacedMerkleTreeConstructor:
    """TreeConstructorFn of rsmt2d's erasured namespaced Merkle tree
    (nmtwrapper_test.go:75-92: celestiaorg/nmt with the parity namespace 0xFF.. for
    every cell outside quadrant 0, IgnoreMaxNamespace).  Recognised by the EDS
    layer, which computes these roots on the GPU (kernels_nmt.hip) for complete
    squares; calling it returns a host Tree like the reference's NewTree."""

    def __init__(self, squareSize: int, namespaceSize: int = 29, ignoreMaxNamespace: bool = True):
        if squareSize == 0:
            raise ValueError("cannot create a erasuredNamespacedMerkleTree of squareSize == 0")
        self.params = NmtParams(namespaceSize, 1 if ignoreMaxNamespace else 0, squareSize)

    def __call__(self, axis: int = Row, index: int = 0) -> Tree:
        return _NmtTree(self.params, axis, index)


def newErasuredNamespacedMerkleTreeConstructor(squareSize: int, namespaceSize: int = 29,
                                               ignoreMaxNamespace: bool = True):
    return ErasuredNamespacedMerkleTreeConstructor(squareSize, namespaceSize, ignoreMaxNamespace)


class BufferedTreeConstructor:
    """tree.go:13-16: NewConstructor(squareSize) -> TreeConstructorFn; TreeCount()."""

    def NewConstructor(self, squareSize: int):  # pragma: no cover - interface
        raise NotImplementedError

    def TreeCount(self) -> int:  # pragma: no cover - interface
        raise NotImplementedError


class TreePool(BufferedTreeConstructor):
    """The pooled NMT of nmtbuffered_tree_test.go:10-58 (newTreePool): a fixed number
    of trees reused across squares of any size.  Its trees push exactly as the
    erasured wrapper does, so here the pool hands out the device-computed NMT
    constructor; TreeCount bounds the host-side root parallelism as setParallelOps
    does (extendeddatasquare.go:90)."""

    def __init__(self, initSquareSize: int, poolSize: int, namespaceSize: int = 29, ignoreMaxNamespace: bool = True):
        if initSquareSize == 0:
            raise ValueError("cannot create a resizeableBufferTree of maxSquareSize == 0")
        self.poolSize, self.namespaceSize, self.ignoreMaxNamespace = poolSize, namespaceSize, ignoreMaxNamespace

    def NewConstructor(self, squareSize: int):
        return ErasuredNamespacedMerkleTreeConstructor(squareSize, self.namespaceSize, self.ignoreMaxNamespace)

    def TreeCount(self) -> int:
        return self.poolSize


def newTreePool(initSquareSize: int, poolSize: int, namespaceSize: int = 29, ignoreMaxNamespace: bool = True):
    return TreePool(initSquareSize, poolSize, namespaceSize, ignoreMaxNamespace)


def _tree_callback(tree_fn):
    """(keep-alive, tree_fn pointer, user pointer) for the C ABI: NULL for
    NewDefaultTree, the library's rsm_nmt_tree_root for the NMT constructor (so the
    GPU computes it), a ctypes callback for any other Python TreeConstructorFn."""
    if tree_fn is None or tree_fn is NewDefaultTree:
        return None, None, None
    if isinstance(tree_fn, ErasuredNamespacedMerkleTreeConstructor):
        fn = ctypes.cast(library().rsm_nmt_tree_root, ctypes.c_void_p)
        return tree_fn.params, fn, ctypes.cast(ctypes.byref(tree_fn.params), ctypes.c_void_p)

    def cb(user, axis, index, leaves, n, leaf_size, root_out, root_len):
        try:
            t = tree_fn(axis, index)
            for i in range(n):
                t.Push(ctypes.string_at(leaves[i], leaf_size))
            r = t.Root()
            if len(r) > root_len[0]:
                return RSM_EINVAL
            ctypes.memmove(root_out, r, len(r))
            root_len[0] = len(r)
            return 0
        except Exception:  # tree errors are byzantine evidence, as in the reference
            return RSM_ETREE

    c = _TREE_FN(cb)
    return c, ctypes.cast(c, ctypes.c_void_p), None


def _default_root(leaves: Sequence[bytes]) -> bytes:
    keep, ptrs, _ = _bufs(leaves)
    out = (ctypes.c_uint8 * 64)()
    ln = ctypes.c_uint32(64)
    _check(library().rsm_default_tree_root(None, 0, 0, ptrs, len(leaves),
                                           len(leaves[0]) if leaves else 0, out, ctypes.byref(ln)))
    return bytes(out[:ln.value])


# ---------------------------------------------------------------------------
# Share inclusion proofs (include/rsmt2d_hip.h "share inclusion proofs")
# ---------------------------------------------------------------------------
class Sample(ctypes.Structure):
    """rsm_sample: leaf ``pos`` of row (axis 0) / column (axis 1) ``index`` of ``square``."""
    _fields_ = [("square", ctypes.c_uint32), ("axis", ctypes.c_uint32), ("index", ctypes.c_uint32),
                ("pos", ctypes.c_uint32)]


def _nmt_ref(nmt: Optional[NmtParams]):
    """The ``const rsm_nmt_params*`` argument: NULL for the DefaultTree."""
    return ctypes.byref(nmt) if nmt is not None else None


def _records(kind, items: Sequence[tuple]):
    """A ctypes array of ``kind`` (Sample, RootRef, NsQuery) from field tuples; one spare
    element when there are none."""
    return (kind * max(len(items), 1))(*[kind(*x) for x in items])


class Proof:
    """A share with its Merkle proof in a row or column tree.

    ``share``: the leaf; ``nodes``: the siblings bottom-up (32-byte digests for the
    DefaultTree, min || max || digest for the NMT); ``right_mask``: bit i set when
    ``nodes[i]`` is the right operand of its parent hash; ``index``: the leaf's
    position; ``numLeaves``: the tree's leaf count; ``root``: the root the proof folds
    to (compare it with the committed row / column root).  ``nmt``: the tree's
    NmtParams, None for the DefaultTree; ``tree_index``: the row / column."""

    def __init__(self, share: bytes, nodes: List[bytes], right_mask: int, index: int, numLeaves: int,
                 nmt: Optional[NmtParams] = None, tree_index: int = 0):
        self.share, self.nodes, self.right_mask = share, nodes, right_mask
        self.index, self.numLeaves, self.nmt, self.tree_index = index, numLeaves, nmt, tree_index

    def proofSet(self) -> List[bytes]:
        """``[share] + nodes``: the proofSet of merkletree.Prove() (treeProve,
        datasquare_test.go:514-537)."""
        return [self.share] + list(self.nodes)

    def nmt_nodes(self) -> List[bytes]:
        """The same nodes in the order of nmt's ``Proof.Nodes`` for the range
        [index, index + 1): an in-order walk -- the left-hand siblings from the top
        down, then the right-hand ones from the bottom up.  The nmt library is not
        available to this project's tests, so parity with it is unpinned, as it is for
        the NMT roots."""
        left = [nd for i, nd in enumerate(self.nodes) if not (self.right_mask >> i) & 1]
        right = [nd for i, nd in enumerate(self.nodes) if (self.right_mask >> i) & 1]
        return left[::-1] + right

    def record(self) -> bytes:
        """The proof record of this proof (include/rsmt2d_hip.h): u32 n_nodes | u32
        right_mask | the nodes | zeros up to 8 + ceil(log2 numLeaves) node lengths --
        the inverse of ``_parse_records``."""
        nl = 32 if self.nmt is None else 2 * int(self.nmt.namespace_size) + 32
        rb = 8 + (self.numLeaves - 1).bit_length() * nl
        body = len(self.nodes).to_bytes(4, "little") + self.right_mask.to_bytes(4, "little") + b"".join(self.nodes)
        if len(body) > rb or any(len(nd) != nl for nd in self.nodes):
            raise RSMError(RSM_EINVAL, "proof nodes do not fit the tree's record")
        return body + bytes(rb - len(body))

    @property
    def root(self) -> bytes:
        import hashlib
        if self.nmt is None:
            acc = hashlib.sha256(b"\x00" + self.share).digest()
            for i, nd in enumerate(self.nodes):
                l, r = (acc, nd) if (self.right_mask >> i) & 1 else (nd, acc)
                acc = hashlib.sha256(b"\x01" + l + r).digest()
            return acc
        ns, k = int(self.nmt.namespace_size), int(self.nmt.square_size)
        nid = self.share[:ns] if (self.index < k and self.tree_index < k) else b"\xff" * ns
        acc = nid + nid + hashlib.sha256(b"\x00" + nid + self.share).digest()
        for i, nd in enumerate(self.nodes):
            l, r = (acc, nd) if (self.right_mask >> i) & 1 else (nd, acc)
            mx = l[ns:2 * ns] if (self.nmt.ignore_max_namespace and r[:ns] == b"\xff" * ns) else r[ns:2 * ns]
            acc = l[:ns] + mx + hashlib.sha256(b"\x01" + l + r).digest()
        return acc


def _parse_records(rec: bytes, shares: bytes, samples, width: int, S: int, nmt: Optional[NmtParams]) -> List[Proof]:
    """Proof objects from n proof records and the n shares; samples: (axis, index, pos)."""
    nl = 32 if nmt is None else 2 * int(nmt.namespace_size) + 32
    levels = (width - 1).bit_length()
    rb = 8 + levels * nl
    out = []
    for i, (_axis, index, pos) in enumerate(samples):
        r = rec[i * rb:(i + 1) * rb]
        n_nodes, mask = int.from_bytes(r[0:4], "little"), int.from_bytes(r[4:8], "little")
        nodes = [r[8 + j * nl: 8 + (j + 1) * nl] for j in range(n_nodes)]
        out.append(Proof(shares[i * S:(i + 1) * S], nodes, mask, pos, width, nmt, index))
    return out


def prove_samples_dev(buf: "DeviceBuffer", width: int, share_size: int, samples: Sequence[tuple],
                      nmt: Optional[NmtParams] = None, count: int = 1) -> List[Proof]:
    """Proofs of ``(square, axis, index, pos)`` samples of ``count`` complete
    device-resident [width][width][share_size] squares in ``buf``: one node-store
    build (rsm_proof_nodes_dev), one gather (rsm_proofs_dev)."""
    L, ctx, n, p = library(), buf.ctx, len(samples), _nmt_ref(nmt)
    nbytes = int(L.rsm_proof_nodes_bytes(width, p, count))
    if nbytes == 0:
        raise RSMError(RSM_EUNSUPPORTED, f"device proofs: {count} squares of width {width} not supported")
    rb = int(L.rsm_proof_record_bytes(width, p))
    nodes, recs, shs = DeviceBuffer(nbytes), DeviceBuffer(max(n * rb, 16)), DeviceBuffer(max(n * share_size, 16))
    try:
        arr = _records(Sample, samples)
        _check(L.rsm_proof_nodes_dev(ctx, buf.ptr, width, share_size, count, p, nodes.ptr, None, None, None))
        _check(L.rsm_proofs_dev(ctx, nodes.ptr, buf.ptr, width, share_size, count, p, arr, n, recs.ptr, shs.ptr, None))
        _check(L.rsm_sync(ctx))
        rec, sh = recs.download(max(n * rb, 16)).tobytes(), shs.download(max(n * share_size, 16)).tobytes()
    finally:
        for b in (nodes, recs, shs):
            b.free()
    return _parse_records(rec, sh, [s[1:] for s in samples], width, share_size, nmt)


def verify_samples_dev(shares: "DeviceBuffer", records: "DeviceBuffer", roots: "DeviceBuffer", width: int,
                       share_size: int, samples: Sequence[tuple], nmt: Optional[NmtParams] = None, count: int = 1):
    """Status words (RSM_PROOF_*) of ``(square, axis, index, pos)`` samples whose shares
    ([n][share_size]) and proof records are device-resident, as rsm_proofs_dev writes
    them, against ``roots`` ([count][2][width][root bytes], as rsm_roots_squares_dev /
    rsm_nmt_roots_squares_dev write them): one rsm_proofs_verify_dev launch."""
    import numpy as np
    L, ctx, n = library(), shares.ctx, len(samples)
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    st = DeviceBuffer(n * 4)
    try:
        _check(L.rsm_proofs_verify_dev(ctx, shares.ptr, records.ptr, roots.ptr, width, share_size, count, _nmt_ref(nmt),
                                       _records(Sample, samples), n, st.ptr, None))
        _check(L.rsm_sync(ctx))
        out[:] = st.download(n * 4).view(np.uint32)
    finally:
        st.free()
    return out


def scatter_samples_dev(eds_buf: "DeviceBuffer", presence_buf: "DeviceBuffer", k: int, share_size: int,
                        samples: Sequence[tuple], shares: "DeviceBuffer", status: "DeviceBuffer", count: int = 1):
    """Sets the verified ones of ``(square, axis, index, pos)`` samples into ``count``
    device-resident [2k][2k][share_size] squares (rsm_samples_scatter_dev): ``shares``
    ([n][share_size]) and ``status`` ([n] uint32, as rsm_proofs_verify_dev wrote it) stay
    on the device; a status-0 sample on a nil cell is copied in and its byte of
    ``presence_buf`` ([count][2k][2k]) set, a status-0 sample on a present cell or behind
    a lower-indexed one of the same cell becomes RSM_PROOF_OCCUPIED.  Returns the status
    words afterwards."""
    import numpy as np
    L, ctx, n = library(), eds_buf.ctx, len(samples)
    if n == 0:
        return np.zeros(0, np.uint32)
    _check(L.rsm_samples_scatter_dev(ctx, eds_buf.ptr, presence_buf.ptr, k, share_size, count, _records(Sample, samples), n,
                                     shares.ptr, status.ptr, None))
    _check(L.rsm_sync(ctx))
    return status.download(n * 4).view(np.uint32).copy()


def _repair_squares(checked: bool, eds_buf, presence_buf, k, share_size, roots_buf, count, nmt):
    """Both device Repair calls: the scratch sized and freed around the call; the result
    records, with ``checked`` also the check records."""
    L, ctx, p = library(), eds_buf.ctx, _nmt_ref(nmt)
    nbytes = int((L.rsm_repair_checked_work_bytes if checked else L.rsm_repair_work_bytes)(k, share_size, count, p))
    if nbytes == 0:
        raise RSMError(RSM_EUNSUPPORTED, f"device repair: {count} squares of width {2 * k} not supported")
    res, chk = (RepairResult * max(count, 1))(), (RepairCheck * max(count, 1))()
    work = DeviceBuffer(nbytes)
    try:
        args = (ctx, eds_buf.ptr, presence_buf.ptr, k, share_size, count, p, roots_buf.ptr, work.ptr, res)
        _check(L.rsm_repair_squares_checked_dev(*args, chk, None) if checked else L.rsm_repair_squares_dev(*args, None))
    finally:
        work.free()
    return list(res[:count]), list(chk[:count])


def repair_squares_dev(eds_buf: "DeviceBuffer", presence_buf: "DeviceBuffer", k: int, share_size: int,
                       roots_buf: "DeviceBuffer", count: int = 1, nmt: Optional[NmtParams] = None) -> List[RepairResult]:
    """Repairs ``count`` device-resident [2k][2k][share_size] squares in place
    (rsm_repair_squares_dev).  ``presence_buf``: [count][2k][2k] bytes, non-zero = given,
    on return the peeling closure; ``roots_buf``: the committed roots
    [count][2][2k][root bytes] as rsm_roots_squares_dev / rsm_nmt_roots_squares_dev write
    them.  One RepairResult per square: status (REPAIR_*), sweeps, decoded_vectors,
    missing.  No attribution of a bad vector: that is ``repair_squares_checked_dev``'s."""
    return _repair_squares(False, eds_buf, presence_buf, k, share_size, roots_buf, count, nmt)[0]


def repair_squares_checked_dev(eds_buf: "DeviceBuffer", presence_buf: "DeviceBuffer", k: int, share_size: int,
                               roots_buf: "DeviceBuffer", count: int = 1, nmt: Optional[NmtParams] = None):
    """``repair_squares_dev`` with attribution (rsm_repair_squares_checked_dev): the same
    decoding passes, and every row and column is checked against its committed root and its
    own encoding in the round in which it first has all 2k cells.  Returns one
    ``(RepairResult, RepairCheck)`` per square.  A square with a bad vector has status
    ``REPAIR_BYZANTINE``; its check names ``axis``, ``index``, ``round`` and ``reason``
    (``BYZ_*``), and its presence bytes are non-zero only in cells that were given or lie
    in vectors that passed: ``byzantine_data_dev`` turns that into ``ErrByzantineData``."""
    return list(zip(*_repair_squares(True, eds_buf, presence_buf, k, share_size, roots_buf, count, nmt)))


def gather_vectors_dev(eds_buf: "DeviceBuffer", presence_buf: "DeviceBuffer", k: int, share_size: int,
                       refs: Sequence[tuple], count: int = 1):
    """The ``(square, axis, index)`` vectors of device squares, packed and downloaded
    (rsm_vectors_gather_dev): ``(shares [n][2k][share_size], present [n][2k])`` uint8."""
    import numpy as np
    L, ctx, n, W = library(), eds_buf.ctx, len(refs), 2 * k
    if n == 0:
        return np.zeros((0, W, share_size), np.uint8), np.zeros((0, W), np.uint8)
    shares, present = DeviceBuffer(n * W * share_size), DeviceBuffer(max(n * W, 16))
    try:
        _check(L.rsm_vectors_gather_dev(ctx, eds_buf.ptr, presence_buf.ptr, k, share_size, count, _records(RootRef, refs), n,
                                        shares.ptr, present.ptr, None))
        _check(L.rsm_sync(ctx))
        return (shares.download(n * W * share_size).reshape(n, W, share_size).copy(),
                present.download(max(n * W, 16))[:n * W].reshape(n, W).copy())
    finally:
        shares.free()
        present.free()


def byzantine_data_dev(eds_buf: "DeviceBuffer", presence_buf: "DeviceBuffer", k: int, share_size: int,
                       outcome: Sequence[tuple], count: int = 1) -> List[Optional[ErrByzantineData]]:
    """``outcome``: what ``repair_squares_checked_dev`` returned for the same buffers.  One
    entry per square: ``ErrByzantineData(Axis, Index, Shares)`` of a ``REPAIR_BYZANTINE``
    square -- the named vector's shares prior to repair, ``None`` where missing -- else
    ``None``.  One gather and one download for the batch."""
    bad = [s for s in range(count) if outcome[s][0].status == REPAIR_BYZANTINE]
    shares, present = gather_vectors_dev(eds_buf, presence_buf, k, share_size,
                                         [(s, outcome[s][1].axis, outcome[s][1].index) for s in bad], count)
    out: List[Optional[ErrByzantineData]] = [None] * count
    for j, s in enumerate(bad):
        out[s] = ErrByzantineData(int(outcome[s][1].axis), int(outcome[s][1].index),
                                  [shares[j, p].tobytes() if present[j, p] else None for p in range(2 * k)])
    return out


# ---------------------------------------------------------------------------
# Bad-encoding fraud proofs (include/rsmt2d_hip.h "bad-encoding fraud proofs")
# ---------------------------------------------------------------------------
def fraud_proof_samples(axis: int, index: int, k: int, square: int = 0) -> List[tuple]:
    """The ``(square, axis ^ 1, j, index)`` samples, j < 2k, whose proofs a fraud proof of
    vector (square, axis, index) carries (rsm_fraud_proof_samples)."""
    out = (Sample * max(2 * k, 1))()
    _check(library().rsm_fraud_proof_samples(ctypes.byref(RootRef(square, axis, index)), k, out))
    return [(s.square, s.axis, s.index, s.pos) for s in out[:2 * k]]


def verify_fraud_proofs_dev(shares: "DeviceBuffer", present: "DeviceBuffer", records: "DeviceBuffer",
                            roots: "DeviceBuffer", k: int, share_size: int, refs: Sequence[tuple], count: int = 1,
                            nmt: Optional[NmtParams] = None) -> List[FraudVerdict]:
    """Validates ``len(refs)`` bad-encoding fraud proofs (rsm_fraud_proofs_verify_dev): proof
    i accuses vector ``refs[i] = (square, axis, index)``; ``shares`` [n][2k][share_size] and
    ``present`` [n][2k] as ``rsm_vectors_gather_dev`` writes them, ``records`` [n][2k] proof
    records of the shares in their orthogonal trees (the samples of ``fraud_proof_samples``),
    ``roots`` the committed table.  One FraudVerdict per proof; the missing slots of
    ``shares`` hold the decoded shares of a FRAUD_VALID or FRAUD_CONSISTENT proof."""
    L, ctx, n, p = library(), shares.ctx, len(refs), _nmt_ref(nmt)
    nbytes = int(L.rsm_fraud_work_bytes(k, share_size, n, p))
    if nbytes == 0:
        raise RSMError(RSM_EUNSUPPORTED, f"fraud proofs: {n} proofs of width {2 * k} not supported")
    out = (FraudVerdict * max(n, 1))()
    work = DeviceBuffer(nbytes)
    try:
        _check(L.rsm_fraud_proofs_verify_dev(ctx, shares.ptr, present.ptr, records.ptr, roots.ptr, k, share_size, count, p,
                                             _records(RootRef, refs), n, work.ptr, out, None))
    finally:
        work.free()
    return list(out[:n])


class BadEncodingProof:
    """The claim that row / column ``index`` (``axis``) of a square is badly encoded: the
    vector's ``shares`` (None where the prover has none) and for each a ``Proof`` in its
    ORTHOGONAL tree -- the reference's PseudoFraudProof (extendeddatacrossword_test.go:19-21)
    with the Merkle proof per share its TODO asks for."""

    def __init__(self, axis: int, index: int, shares: Sequence[Optional[bytes]], proofs: Sequence[Optional["Proof"]]):
        self.axis, self.index, self.shares, self.proofs = axis, index, list(shares), list(proofs)

    def Validate(self, rowRoots: Sequence[bytes], colRoots: Sequence[bytes], codec: Codec,
                 treeCreatorFn=NewDefaultTree) -> FraudVerdict:
        """The verdict of this proof against the committed roots, decided on the device of
        ``codec``: FRAUD_VALID (with ``reason``) when the proof holds."""
        import numpy as np
        nmt = treeCreatorFn.params if isinstance(treeCreatorFn, ErasuredNamespacedMerkleTreeConstructor) else None
        W = len(self.shares)
        have = [s for s in self.shares if s is not None]
        if W == 0 or W % 2 or len(self.proofs) != W or not have or len(rowRoots) != W or len(colRoots) != W:
            raise RSMError(RSM_EINVAL, "a fraud proof carries 2k slots, a share in one at least, and 2k roots per axis")
        S = len(have[0])
        rb = int(library().rsm_proof_record_bytes(W, _nmt_ref(nmt)))
        sh, pr, rec = np.zeros((W, S), np.uint8), np.zeros(W, np.uint8), np.zeros((W, rb), np.uint8)
        for j, (s, p) in enumerate(zip(self.shares, self.proofs)):
            if s is None:
                continue
            if len(s) != S or p is None:
                raise RSMError(RSM_EINVAL, "every share of a fraud proof has the same size and a proof")
            sh[j], pr[j], rec[j] = np.frombuffer(s, np.uint8), 1, np.frombuffer(p.record(), np.uint8)
        table = np.frombuffer(b"".join(bytes(r) for r in list(rowRoots) + list(colRoots)), np.uint8)
        dev = _device_of(codec)
        bufs = [DeviceBuffer(max(a.nbytes, 16), dev) for a in (sh, pr, rec, table)]
        try:
            for b, a in zip(bufs, (sh, pr, rec, table)):
                b.upload(a.reshape(-1))
            return verify_fraud_proofs_dev(*bufs, W // 2, S, [(0, self.axis, self.index)], 1, nmt)[0]
        finally:
            for b in bufs:
                b.free()


# ---------------------------------------------------------------------------
# Data root (include/rsmt2d_hip.h "data root")
# ---------------------------------------------------------------------------
class RootRef(ctypes.Structure):
    """rsm_root_ref: the root of row (axis 0) / column (axis 1) ``index`` of ``square``."""
    _fields_ = [("square", ctypes.c_uint32), ("axis", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class RootProof:
    """The proof of one row or column root under a square's data root (the RFC 6962 root
    over rowRoots ++ colRoots, DataAvailabilityHeader.Hash()).

    ``nodes``: the 32-byte siblings bottom-up; ``right_mask``: bit i set when ``nodes[i]``
    is the right operand of its parent hash; ``axis`` / ``index``: the root proven, leaf
    ``axis * width + index`` of the tree over ``2 * width`` roots."""

    def __init__(self, nodes: List[bytes], right_mask: int, axis: int, index: int, width: int):
        self.nodes, self.right_mask, self.axis, self.index, self.width = nodes, right_mask, axis, index, width

    def record(self) -> bytes:
        """The root proof record (include/rsmt2d_hip.h): u32 n_nodes | u32 right_mask | the
        nodes | zeros up to 8 + ceil(log2(2 width)) * 32 bytes."""
        rb = 8 + (2 * self.width - 1).bit_length() * 32
        body = len(self.nodes).to_bytes(4, "little") + self.right_mask.to_bytes(4, "little") + b"".join(self.nodes)
        if len(body) > rb or any(len(nd) != 32 for nd in self.nodes):
            raise RSMError(RSM_EINVAL, "proof nodes do not fit the data-root tree's record")
        return body + bytes(rb - len(body))

    def verify(self, root_bytes: bytes, data_root: bytes) -> int:
        """The status word (RSM_PROOF_*) of ``root_bytes`` as this proof's leaf under
        ``data_root`` (rsm_data_root_verify)."""
        st = ctypes.c_uint32(0)
        _check(library().rsm_data_root_verify(bytes(root_bytes), len(root_bytes), self.width, self.axis, self.index,
                                              self.record(), bytes(data_root), ctypes.byref(st)))
        return int(st.value)


def _parse_root_records(rec: bytes, refs, width: int) -> List[RootProof]:
    """RootProof objects from n root proof records; refs: (axis, index)."""
    rb = 8 + (2 * width - 1).bit_length() * 32
    out = []
    for i, (axis, index) in enumerate(refs):
        r = rec[i * rb:(i + 1) * rb]
        n_nodes, mask = int.from_bytes(r[0:4], "little"), int.from_bytes(r[4:8], "little")
        out.append(RootProof([r[8 + j * 32: 8 + (j + 1) * 32] for j in range(n_nodes)], mask, axis, index, width))
    return out


def data_roots_dev(roots_buf: "DeviceBuffer", width: int, root_len: int, count: int, want_nodes: bool = False):
    """The data roots of ``count`` squares whose roots ([count][2][width][root_len], as the
    roots calls write them) are device-resident in ``roots_buf``: one rsm_data_roots_dev
    launch.  Returns a (count, 32) uint8 array; with ``want_nodes`` also the node store (a
    DeviceBuffer the caller frees) for ``prove_roots_dev``."""
    import numpy as np
    L, ctx = library(), roots_buf.ctx
    nbytes = int(L.rsm_data_root_nodes_bytes(width, count)) if want_nodes else 0
    if want_nodes and nbytes == 0 and count:
        raise RSMError(RSM_EUNSUPPORTED, f"device data roots: width {width} not supported")
    out = DeviceBuffer(max(count * 32, 16))
    nodes = DeviceBuffer(max(nbytes, 16)) if want_nodes else None
    try:
        _check(L.rsm_data_roots_dev(ctx, roots_buf.ptr, width, root_len, count, out.ptr,
                                    nodes.ptr if nodes is not None else None, None))
        _check(L.rsm_sync(ctx))
        got = out.download(max(count * 32, 16))[:count * 32].reshape(count, 32).copy()
    except Exception:
        if nodes is not None:
            nodes.free()
        raise
    finally:
        out.free()
    return (got, nodes) if want_nodes else got


def prove_roots_dev(nodes: "DeviceBuffer", width: int, refs: Sequence[tuple], count: int = 1) -> List[RootProof]:
    """Proofs of the ``(square, axis, index)`` roots out of the node store that
    ``data_roots_dev(..., want_nodes=True)`` returned: one rsm_root_proofs_dev gather."""
    L, ctx, n = library(), nodes.ctx, len(refs)
    rb = int(L.rsm_data_root_record_bytes(width))
    recs = DeviceBuffer(max(n * rb, 16))
    try:
        _check(L.rsm_root_proofs_dev(ctx, nodes.ptr, width, count, _records(RootRef, refs), n, recs.ptr, None))
        _check(L.rsm_sync(ctx))
        rec = recs.download(max(n * rb, 16)).tobytes()
    finally:
        recs.free()
    return _parse_root_records(rec, [r[1:] for r in refs], width)


def verify_samples_data_root_dev(shares: "DeviceBuffer", records: "DeviceBuffer", root_records: "DeviceBuffer",
                                 data_roots: "DeviceBuffer", width: int, share_size: int, samples: Sequence[tuple],
                                 nmt: Optional[NmtParams] = None, count: int = 1):
    """Status words (RSM_PROOF_*) of ``(square, axis, index, pos)`` samples checked all the
    way to their square's data root, with no root table: shares, share proof records and
    root proof records device-resident as rsm_proofs_dev / rsm_root_proofs_dev write them,
    ``data_roots`` [count][32]: one rsm_proofs_verify_data_root_dev launch."""
    import numpy as np
    L, ctx, n = library(), shares.ctx, len(samples)
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    st = DeviceBuffer(n * 4)
    try:
        _check(L.rsm_proofs_verify_data_root_dev(ctx, shares.ptr, records.ptr, root_records.ptr, data_roots.ptr, width,
                                                 share_size, count, _nmt_ref(nmt), _records(Sample, samples), n, st.ptr,
                                                 None))
        _check(L.rsm_sync(ctx))
        out[:] = st.download(n * 4).view(np.uint32)
    finally:
        st.free()
    return out


# ---------------------------------------------------------------------------
# Namespace proofs (include/rsmt2d_hip.h "namespace proofs")
# ---------------------------------------------------------------------------
#: NamespaceProof.kind
NS_EMPTY, NS_INCLUSION, NS_ABSENCE, NS_TREE = 0, 1, 2, 3


class NsQuery(ctypes.Structure):
    """rsm_ns_query: row (axis 0) / column (axis 1) ``index`` of ``square``."""
    _fields_ = [("square", ctypes.c_uint32), ("axis", ctypes.c_uint32), ("index", ctypes.c_uint32)]


class NamespaceProof:
    """Every share of one namespace in a row or column, with the proof that these are
    all of them (nmt's ProveNamespace).

    ``kind``: NS_EMPTY (the namespace lies outside the root's range: nothing to show),
    NS_INCLUSION (``shares`` are leaves ``start`` .. ``end - 1``), NS_ABSENCE
    (``leaf_node`` is the node of leaf ``start``, the first one above the namespace) or
    NS_TREE (device batches only: the tree fails, there is no proof).  ``nodes``: the
    range proof of [start, end) in nmt's ``Proof.Nodes`` order.  ``numLeaves``,
    ``nmt``, ``tree_index``: the tree, as in ``Proof``."""

    def __init__(self, kind: int, start: int, end: int, nodes: List[bytes], leaf_node: Optional[bytes],
                 shares: List[bytes], numLeaves: int, nmt: NmtParams, tree_index: int = 0):
        self.kind, self.start, self.end, self.nodes = kind, start, end, nodes
        self.leaf_node, self.shares = leaf_node, shares
        self.numLeaves, self.nmt, self.tree_index = numLeaves, nmt, tree_index

    def record(self) -> bytes:
        """The namespace proof record (include/rsmt2d_hip.h): u32 kind | start | end |
        n_nodes | the nodes | zeros up to slot 2L | the leaf node or zeros."""
        nl = 2 * int(self.nmt.namespace_size) + 32
        levels = (self.numLeaves - 1).bit_length()
        if len(self.nodes) > 2 * levels or any(len(nd) != nl for nd in self.nodes) or \
                (self.leaf_node is not None and len(self.leaf_node) != nl):
            raise RSMError(RSM_EINVAL, "proof nodes do not fit the tree's record")
        head = b"".join(int(v).to_bytes(4, "little") for v in (self.kind, self.start, self.end, len(self.nodes)))
        body = b"".join(self.nodes)
        return head + body + bytes(2 * levels * nl - len(body)) + (self.leaf_node or bytes(nl))

    def verify(self, root: bytes, nid: bytes) -> int:
        """The RSM_PROOF_* status of this proof for namespace ``nid`` against the
        committed ``root`` (rsm_nmt_namespace_verify): 0 = these are all the shares."""
        ns = int(self.nmt.namespace_size)
        if len(nid) != ns or len(root) != 2 * ns + 32:
            raise RSMError(RSM_EINVAL, "namespace or root of the wrong length")
        S = len(self.shares[0]) if self.shares else 0
        if any(len(sh) != S for sh in self.shares):
            raise RSMError(RSM_EINVAL, "shares of different sizes")
        st = ctypes.c_uint32(0)
        _check(library().rsm_nmt_namespace_verify(ctypes.byref(self.nmt), self.tree_index, bytes(nid),
                                                  b"".join(self.shares), len(self.shares), S, self.numLeaves,
                                                  self.record(), bytes(root), ctypes.byref(st)))
        return int(st.value)


def _parse_ns_records(rec: bytes, offsets, shares: Optional[bytes], indices, width: int, S: int,
                      nmt: NmtParams) -> List[NamespaceProof]:
    """NamespaceProof objects from n records, the n + 1 offsets and the packed shares."""
    nl = 2 * int(nmt.namespace_size) + 32
    levels = (width - 1).bit_length()
    rb = 16 + (2 * levels + 1) * nl
    out = []
    for i, index in enumerate(indices):
        r = rec[i * rb:(i + 1) * rb]
        kind, start, end, n_nodes = (int.from_bytes(r[4 * j:4 * j + 4], "little") for j in range(4))
        nodes = [r[16 + j * nl: 16 + (j + 1) * nl] for j in range(n_nodes)]
        leaf = r[16 + 2 * levels * nl:] if kind == NS_ABSENCE else None
        sh = [shares[p * S:(p + 1) * S] for p in range(int(offsets[i]), int(offsets[i + 1]))]
        out.append(NamespaceProof(kind, start, end, nodes, leaf, sh, width, nmt, index))
    return out


def prove_namespaces_dev(buf: "DeviceBuffer", width: int, share_size: int, queries: Sequence[tuple],
                         nids: Sequence[bytes], nmt: NmtParams, count: int = 1) -> List[NamespaceProof]:
    """Namespace proofs of ``(square, axis, index)`` queries, query i for namespace
    ``nids[i]``, of ``count`` complete device-resident [width][width][share_size] squares
    in ``buf``: one node-store build (rsm_proof_nodes_dev), then rsm_ns_proofs_dev once
    for the records and the share total and once more with a share buffer of that size."""
    import numpy as np
    L, ctx, n = library(), buf.ctx, len(queries)
    if nmt is None:
        raise RSMError(RSM_EUNSUPPORTED, "namespace proofs need the NMT")
    p, ns = ctypes.byref(nmt), int(nmt.namespace_size)
    if len(nids) != n or any(len(x) != ns for x in nids):
        raise RSMError(RSM_EINVAL, "one namespace of namespace_size bytes per query")
    nbytes = int(L.rsm_proof_nodes_bytes(width, p, count))
    if nbytes == 0:
        raise RSMError(RSM_EUNSUPPORTED, f"device proofs: {count} squares of width {width} not supported")
    if n == 0:
        return []
    rb = int(L.rsm_ns_record_bytes(width, p))
    bufs = [DeviceBuffer(nbytes), DeviceBuffer(count * 2 * width * 4), DeviceBuffer(n * rb), DeviceBuffer((n + 1) * 4)]
    nodes, status, recs, offs = bufs
    try:
        arr = _records(NsQuery, queries)
        flat = b"".join(bytes(x) for x in nids)
        _check(L.rsm_proof_nodes_dev(ctx, buf.ptr, width, share_size, count, p, nodes.ptr, None, status.ptr, None))
        _check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, status.ptr, buf.ptr, width, share_size, count, p, arr, flat, n,
                                   recs.ptr, offs.ptr, None, 0, None))
        _check(L.rsm_sync(ctx))
        offsets = offs.download((n + 1) * 4).view(np.uint32).copy()
        total = int(offsets[n])
        sh = b""
        if total:
            shs = DeviceBuffer(total * share_size)
            bufs.append(shs)
            _check(L.rsm_ns_proofs_dev(ctx, nodes.ptr, status.ptr, buf.ptr, width, share_size, count, p, arr, flat, n,
                                       recs.ptr, offs.ptr, shs.ptr, total, None))
            _check(L.rsm_sync(ctx))
            sh = shs.download(total * share_size).tobytes()
        rec = recs.download(n * rb).tobytes()
    finally:
        for b in bufs:
            b.free()
    return _parse_ns_records(rec, offsets, sh, [q[2] for q in queries], width, share_size, nmt)


def verify_namespaces_dev(records: "DeviceBuffer", offsets: "DeviceBuffer", shares: Optional["DeviceBuffer"],
                          shares_total: int, roots: "DeviceBuffer", width: int, share_size: int,
                          queries: Sequence[tuple], nids: Sequence[bytes], nmt: NmtParams, count: int = 1):
    """Status words (RSM_PROOF_*) of ``(square, axis, index)`` queries, query i for
    namespace ``nids[i]``, whose records, offsets and packed shares are device-resident as
    rsm_ns_proofs_dev writes them, against ``roots`` ([count][2][width][root bytes], as
    rsm_nmt_roots_squares_dev writes them): one rsm_ns_proofs_verify_dev launch, one wave
    per query.  0 = these are all the shares of that namespace in that vector."""
    import numpy as np
    L, ctx, n = library(), records.ctx, len(queries)
    if nmt is None:
        raise RSMError(RSM_EUNSUPPORTED, "namespace proofs need the NMT")
    ns = int(nmt.namespace_size)
    if len(nids) != n or any(len(x) != ns for x in nids):
        raise RSMError(RSM_EINVAL, "one namespace of namespace_size bytes per query")
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    st = DeviceBuffer(n * 4)
    try:
        _check(L.rsm_ns_proofs_verify_dev(ctx, records.ptr, offsets.ptr, shares.ptr if shares is not None else None,
                                          shares_total, roots.ptr, width, share_size, count, ctypes.byref(nmt),
                                          _records(NsQuery, queries), b"".join(bytes(x) for x in nids), n, st.ptr, None))
        _check(L.rsm_sync(ctx))
        out[:] = st.download(n * 4).view(np.uint32)
    finally:
        st.free()
    return out


# ---------------------------------------------------------------------------
# Range proofs (include/rsmt2d_hip.h "range proofs")
# ---------------------------------------------------------------------------
class RangeQuery(ctypes.Structure):
    """rsm_range_query: leaves [``start``, ``end``) of row (axis 0) / column (axis 1)
    ``index`` of ``square``."""
    _fields_ = [("square", ctypes.c_uint32), ("axis", ctypes.c_uint32), ("index", ctypes.c_uint32),
                ("start", ctypes.c_uint32), ("end", ctypes.c_uint32)]


class RangeProof:
    """Shares ``start`` .. ``end - 1`` of a row or column with their proof under its root
    (nmt's ProveRange; one row of Celestia's ShareProof).

    ``nodes``: the range proof of [start, end) in nmt's ``Proof.Nodes`` order;
    ``numLeaves``, ``nmt`` (None: DefaultTree), ``axis``, ``tree_index``: the tree."""

    def __init__(self, start: int, end: int, nodes: List[bytes], shares: List[bytes], numLeaves: int,
                 nmt: Optional[NmtParams] = None, axis: int = 0, tree_index: int = 0):
        self.start, self.end, self.nodes, self.shares = start, end, nodes, shares
        self.numLeaves, self.nmt, self.axis, self.tree_index = numLeaves, nmt, axis, tree_index

    def record(self) -> bytes:
        """The range proof record (include/rsmt2d_hip.h): u32 kind = 1 | start | end |
        n_nodes | the nodes | zeros up to and including slot 2L."""
        nl = 2 * int(self.nmt.namespace_size) + 32 if self.nmt is not None else 32
        levels = (self.numLeaves - 1).bit_length()
        if len(self.nodes) > 2 * levels or any(len(nd) != nl for nd in self.nodes):
            raise RSMError(RSM_EINVAL, "proof nodes do not fit the tree's record")
        head = b"".join(int(v).to_bytes(4, "little") for v in (NS_INCLUSION, self.start, self.end, len(self.nodes)))
        body = b"".join(self.nodes)
        return head + body + bytes((2 * levels + 1) * nl - len(body))

    def verify(self, root: bytes) -> int:
        """The RSM_PROOF_* status of ``shares`` as leaves [start, end) under the committed
        ``root`` (rsm_default_tree_range_verify / rsm_nmt_tree_range_verify)."""
        S = len(self.shares[0]) if self.shares else 0
        if any(len(sh) != S for sh in self.shares):
            raise RSMError(RSM_EINVAL, "shares of different sizes")
        st, L = ctypes.c_uint32(0), library()
        flat = b"".join(self.shares)
        if self.nmt is None:
            _check(L.rsm_default_tree_range_verify(self.start, self.end, flat, len(self.shares), S, self.numLeaves,
                                                   self.record(), bytes(root), ctypes.byref(st)))
        else:
            _check(L.rsm_nmt_tree_range_verify(ctypes.byref(self.nmt), self.tree_index, self.start, self.end, flat,
                                               len(self.shares), S, self.numLeaves, self.record(), bytes(root),
                                               ctypes.byref(st)))
        return int(st.value)


def _parse_range_records(rec: bytes, offsets, shares: bytes, queries, width: int, S: int,
                         nmt: Optional[NmtParams]) -> List[RangeProof]:
    """RangeProof objects from n records, the n + 1 offsets and the packed shares; queries:
    (axis, index, start, end)."""
    nl = 2 * int(nmt.namespace_size) + 32 if nmt is not None else 32
    rb = 16 + (2 * (width - 1).bit_length() + 1) * nl
    out = []
    for i, (axis, index, start, end) in enumerate(queries):
        r = rec[i * rb:(i + 1) * rb]
        n_nodes = int.from_bytes(r[12:16], "little")
        nodes = [r[16 + j * nl: 16 + (j + 1) * nl] for j in range(n_nodes)]
        sh = [shares[p * S:(p + 1) * S] for p in range(int(offsets[i]), int(offsets[i + 1]))]
        out.append(RangeProof(start, end, nodes, sh, width, nmt, axis, index))
    return out


def share_range_queries(k: int, start: int, end: int, square: int = 0) -> List[tuple]:
    """ODS shares [start, end) in row-major order of the k x k original square as one
    ``(square, Row, row, first, last + 1)`` query per touched row (rsm_share_range_queries)."""
    out = (RangeQuery * max(k, 1))()
    n = ctypes.c_uint32(0)
    _check(library().rsm_share_range_queries(k, square, start, end, out, ctypes.byref(n)))
    return [(q.square, q.axis, q.index, q.start, q.end) for q in out[:n.value]]


def prove_ranges_dev(buf: "DeviceBuffer", width: int, share_size: int, queries: Sequence[tuple],
                     nmt: Optional[NmtParams] = None, count: int = 1) -> List[RangeProof]:
    """Range proofs of ``(square, axis, index, start, end)`` queries of ``count`` complete
    device-resident [width][width][share_size] squares in ``buf``: one node-store build
    (rsm_proof_nodes_dev) and one rsm_range_proofs_dev (the share total is known up front)."""
    import numpy as np
    L, ctx, n = library(), buf.ctx, len(queries)
    p = _nmt_ref(nmt)
    nbytes = int(L.rsm_proof_nodes_bytes(width, p, count))
    if nbytes == 0:
        raise RSMError(RSM_EUNSUPPORTED, f"device proofs: {count} squares of width {width} not supported")
    if n == 0:
        return []
    rb = int(L.rsm_range_record_bytes(width, p))
    total = sum(max(int(q[4]) - int(q[3]), 0) for q in queries)
    bufs = [DeviceBuffer(nbytes), DeviceBuffer(n * rb), DeviceBuffer((n + 1) * 4), DeviceBuffer(max(total * share_size, 16))]
    nodes, recs, offs, shs = bufs
    try:
        _check(L.rsm_proof_nodes_dev(ctx, buf.ptr, width, share_size, count, p, nodes.ptr, None, None, None))
        _check(L.rsm_range_proofs_dev(ctx, nodes.ptr, buf.ptr, width, share_size, count, p, _records(RangeQuery, queries), n,
                                      recs.ptr, offs.ptr, shs.ptr, total, None))
        _check(L.rsm_sync(ctx))
        offsets = offs.download((n + 1) * 4).view(np.uint32).copy()
        sh = shs.download(max(total * share_size, 16)).tobytes()
        rec = recs.download(n * rb).tobytes()
    finally:
        for b in bufs:
            b.free()
    return _parse_range_records(rec, offsets, sh, [q[1:] for q in queries], width, share_size, nmt)


def _verify_ranges(call, records, offsets, shares, shares_total, against, width, share_size, queries, nmt, count):
    import numpy as np
    L, ctx, n = library(), records.ctx, len(queries)
    out = np.zeros(n, np.uint32)
    if n == 0:
        return out
    st = DeviceBuffer(n * 4)
    try:
        _check(getattr(L, call)(ctx, records.ptr, offsets.ptr, shares.ptr if shares is not None else None, shares_total,
                                *[b.ptr for b in against], width, share_size, count, _nmt_ref(nmt),
                                _records(RangeQuery, queries), n, st.ptr, None))
        _check(L.rsm_sync(ctx))
        out[:] = st.download(n * 4).view(np.uint32)
    finally:
        st.free()
    return out


def verify_ranges_dev(records: "DeviceBuffer", offsets: "DeviceBuffer", shares: Optional["DeviceBuffer"],
                      shares_total: int, roots: "DeviceBuffer", width: int, share_size: int, queries: Sequence[tuple],
                      nmt: Optional[NmtParams] = None, count: int = 1):
    """Status words (RSM_PROOF_*) of ``(square, axis, index, start, end)`` queries whose
    records, offsets and packed shares are device-resident as rsm_range_proofs_dev writes
    them, against ``roots`` ([count][2][width][root bytes]): one
    rsm_range_proofs_verify_dev launch, one wave per query.  0 = these shares are leaves
    [start, end) of that vector."""
    return _verify_ranges("rsm_range_proofs_verify_dev", records, offsets, shares, shares_total, [roots], width, share_size,
                          queries, nmt, count)


def verify_ranges_data_root_dev(records: "DeviceBuffer", offsets: "DeviceBuffer", shares: Optional["DeviceBuffer"],
                                shares_total: int, root_records: "DeviceBuffer", data_roots: "DeviceBuffer", width: int,
                                share_size: int, queries: Sequence[tuple], nmt: Optional[NmtParams] = None, count: int = 1):
    """The same all the way to each square's data root, with no root table: query i also
    takes root proof record i of ``root_records`` (as rsm_root_proofs_dev writes them) and
    ``data_roots`` [count][32]: one rsm_range_proofs_verify_data_root_dev launch."""
    return _verify_ranges("rsm_range_proofs_verify_data_root_dev", records, offsets, shares, shares_total,
                          [root_records, data_roots], width, share_size, queries, nmt, count)


# ---------------------------------------------------------------------------
# Share commitments (include/rsmt2d_hip.h "share commitments")
# ---------------------------------------------------------------------------
class BlobRef(ctypes.Structure):
    """rsm_blob_ref: ODS shares [start, start + len) of ``square``, row-major."""
    _fields_ = [("square", ctypes.c_uint32), ("start", ctypes.c_uint32), ("len", ctypes.c_uint32)]


def SubTreeWidth(shareCount: int, subtreeRootThreshold: int = 64) -> int:
    """celestia-app's inclusion.SubTreeWidth (rsm_subtree_width)."""
    return int(library().rsm_subtree_width(shareCount, subtreeRootThreshold))


def MerkleMountainRangeSizes(totalSize: int, maxTreeSize: int) -> List[int]:
    """celestia-app's inclusion.MerkleMountainRangeSizes (rsm_subtree_sizes)."""
    if totalSize == 0:
        return []
    L, m = library(), ctypes.c_uint32(0)
    _check(L.rsm_subtree_sizes(totalSize, maxTreeSize, None, 0, ctypes.byref(m)))
    out = (ctypes.c_uint32 * m.value)()
    _check(L.rsm_subtree_sizes(totalSize, maxTreeSize, out, m.value, ctypes.byref(m)))
    return list(out)


def _commit_error(status: int) -> RSMError:
    return RSMError(RSM_ETREE, "share commitment: namespaces out of order (status %d)" % status)


def blob_commitments_dev(shares: "DeviceBuffer", share_size: int, offsets: Sequence[int], nmt: NmtParams,
                         threshold: int = 64):
    """(commitments [n][32], status words [n]) of the n blobs whose shares are
    [offsets[i], offsets[i + 1]) of the packed device-resident ``shares``: one
    rsm_blob_commitments_dev call (leaf pass, subtree pass, fold)."""
    import numpy as np
    L, ctx, n = library(), shares.ctx, len(offsets) - 1
    com, st = np.zeros((max(n, 0), 32), np.uint8), np.zeros(max(n, 0), np.uint32)
    if n <= 0:
        return com, st
    offs = (ctypes.c_uint32 * (n + 1))(*[int(o) for o in offsets])
    lens = [int(offsets[i + 1]) - int(offsets[i]) for i in range(n)]
    total = int(offsets[n]) - int(offsets[0])
    roots = sum(len(MerkleMountainRangeSizes(x, SubTreeWidth(x, threshold))) for x in lens if x > 0)
    wb = int(L.rsm_commit_work_bytes(max(total, 0), roots, _nmt_ref(nmt)))
    bufs = [DeviceBuffer(max(wb, 16)), DeviceBuffer(n * 32), DeviceBuffer(n * 4)]
    work, dc, ds = bufs
    try:
        _check(L.rsm_blob_commitments_dev(ctx, shares.ptr, share_size, _nmt_ref(nmt), threshold, offs, n, work.ptr, dc.ptr,
                                          ds.ptr, None))
        _check(L.rsm_sync(ctx))
        com[:] = dc.download(n * 32).reshape(n, 32)
        st[:] = ds.download(n * 4).view(np.uint32)
    finally:
        for b in bufs:
            b.free()
    return com, st


def commitments_dev(nodes: "DeviceBuffer", status_trees: "DeviceBuffer", width: int, blobs: Sequence[tuple], nmt: NmtParams,
                    threshold: int = 64, count: int = 1, want_roots: bool = False):
    """(commitments [n][32], status words [n]) of ``(square, start, len)`` blobs out of the
    NMT node store and tree status words rsm_proof_nodes_dev wrote: one rsm_commitments_dev
    call, no share read.  ``want_roots``: also each blob's list of subtree roots."""
    import numpy as np
    L, ctx, n = library(), nodes.ctx, len(blobs)
    com, st = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint32)
    if n == 0:
        return (com, st, []) if want_roots else (com, st)
    nl = 2 * nmt.namespace_size + 32
    counts = [len(MerkleMountainRangeSizes(int(b[2]), SubTreeWidth(int(b[2]), threshold))) for b in blobs]
    bufs = [DeviceBuffer(n * 32), DeviceBuffer(n * 4)]
    if want_roots:
        bufs += [DeviceBuffer(max(sum(counts) * nl, 16)), DeviceBuffer((n + 1) * 4)]
    try:
        _check(L.rsm_commitments_dev(ctx, nodes.ptr, status_trees.ptr, width, count, _nmt_ref(nmt), threshold,
                                     _records(BlobRef, blobs), n, bufs[2].ptr if want_roots else None,
                                     bufs[3].ptr if want_roots else None, bufs[0].ptr, bufs[1].ptr, None))
        _check(L.rsm_sync(ctx))
        com[:] = bufs[0].download(n * 32).reshape(n, 32)
        st[:] = bufs[1].download(n * 4).view(np.uint32)
        if want_roots:
            offs = bufs[3].download((n + 1) * 4).view(np.uint32)
            raw = bufs[2].download(max(sum(counts) * nl, 16)).tobytes()
            roots = [[raw[j * nl:(j + 1) * nl] for j in range(int(offs[i]), int(offs[i + 1]))] for i in range(n)]
            return com, st, roots
    finally:
        for b in bufs:
            b.free()
    return com, st


def CreateCommitment(shares: Sequence[bytes], nmt: NmtParams, threshold: int = 64, device: Optional[int] = 0) -> bytes:
    """celestia-app's inclusion.CreateCommitment over a blob's shares: the 32-byte share
    commitment of a MsgPayForBlobs.  On the GPU (rsm_blob_commitments_dev); with
    ``device=None`` the host restatement (rsm_blob_commitment).  Raises RSMError(RSM_ETREE)
    where a subtree's namespaces are out of order."""
    import numpy as np
    n, S = len(shares), len(shares[0]) if shares else 0
    if n == 0 or any(len(s) != S for s in shares):
        raise RSMError(RSM_EINVAL, "CreateCommitment: a blob is one or more shares of one size")
    flat = b"".join(shares)
    if device is None:
        out, st = ctypes.create_string_buffer(32), ctypes.c_uint32(0)
        _check(library().rsm_blob_commitment(_nmt_ref(nmt), flat, n, S, threshold, out, ctypes.byref(st)))
        if st.value:
            raise _commit_error(st.value)
        return out.raw
    buf = DeviceBuffer(max(len(flat), 16), device)
    try:
        buf.upload(np.frombuffer(flat, np.uint8))
        com, st = blob_commitments_dev(buf, S, [0, n], nmt, threshold)
    finally:
        buf.free()
    if st[0]:
        raise _commit_error(int(st[0]))
    return com[0].tobytes()


class ShareProof:
    """ODS shares [start, end) of a square under its data root (Celestia's ShareProof): per
    touched row a ``RangeProof`` and the ``RootProof`` of that row's root; ``row_roots``:
    the row roots the range proofs fold to."""

    def __init__(self, start: int, end: int, rows: List[RangeProof], root_proofs: List[RootProof], row_roots: List[bytes]):
        self.start, self.end, self.rows, self.root_proofs, self.row_roots = start, end, rows, root_proofs, row_roots

    def shares(self) -> List[bytes]:
        return [sh for pr in self.rows for sh in pr.shares]

    def statuses(self, dataRoot: bytes, device: Optional[int] = 0) -> List[int]:
        """One RSM_PROOF_* status per row for the chained check against ``dataRoot``: one
        rsm_range_proofs_verify_data_root_dev call on GPU ``device``; ``device=None``
        verifies each range against its row root and that root under ``dataRoot`` on the
        host.  Results never depend on the path."""
        import numpy as np
        if not self.rows or len(self.rows) != len(self.root_proofs) or len(self.rows) != len(self.row_roots):
            raise RSMError(RSM_EINVAL, "a ShareProof has one range proof, root proof and row root per row")
        if device is None:
            out = []
            for pr, rp, root in zip(self.rows, self.root_proofs, self.row_roots):
                st = pr.verify(root)
                out.append(st if st != RSM_PROOF_OK else RootProof(rp.nodes, rp.right_mask, pr.axis, pr.tree_index,
                                                                    pr.numLeaves).verify(root, dataRoot))
            return out
        w, nmt = self.rows[0].numLeaves, self.rows[0].nmt
        sizes = {len(sh) for pr in self.rows for sh in pr.shares}
        if len(sizes) > 1 or any(pr.numLeaves != w for pr in self.rows):
            raise RSMError(RSM_EINVAL, "shares of different sizes or rows of different squares")
        S = sizes.pop() if sizes else 64
        offsets = np.cumsum([0] + [len(pr.shares) for pr in self.rows]).astype(np.uint32)
        total = int(offsets[-1])
        recs = b"".join(pr.record() for pr in self.rows)
        rrecs = b"".join(RootProof(rp.nodes, rp.right_mask, rp.axis, rp.index, w).record() for rp in self.root_proofs)
        bufs = [DeviceBuffer(len(recs), device), DeviceBuffer(offsets.nbytes, device), DeviceBuffer(max(total * S, 16), device),
                DeviceBuffer(len(rrecs), device), DeviceBuffer(32, device)]
        try:
            bufs[0].upload(np.frombuffer(recs, np.uint8))
            bufs[1].upload(offsets.view(np.uint8))
            if total:
                bufs[2].upload(np.frombuffer(b"".join(self.shares()), np.uint8))
            bufs[3].upload(np.frombuffer(rrecs, np.uint8))
            bufs[4].upload(np.frombuffer(bytes(dataRoot), np.uint8))
            st = verify_ranges_data_root_dev(bufs[0], bufs[1], bufs[2], total, bufs[3], bufs[4], w, S,
                                             [(0, pr.axis, pr.tree_index, pr.start, pr.end) for pr in self.rows], nmt)
            return [int(x) for x in st]
        finally:
            for b in bufs:
                b.free()

    def Validate(self, dataRoot: bytes, device: Optional[int] = 0) -> bool:
        """True iff every row's chained check against ``dataRoot`` is RSM_PROOF_OK."""
        if len(dataRoot) != 32:
            raise RSMError(RSM_EINVAL, "a data root of 32 bytes is needed")
        return all(st == RSM_PROOF_OK for st in self.statuses(dataRoot, device))


def verify_namespace_data(row_roots: Sequence[bytes], nid: bytes, data: Sequence[tuple], nmt: NmtParams, width: int,
                          device: Optional[int] = 0) -> List[int]:
    """The client side of ``ExtendedDataSquare.NamespaceData``: one RSM_PROOF_* status per
    row of the square for the answer ``data`` (``(rowIdx, NamespaceProof)`` pairs) to
    "every share of ``nid``", against the committed ``row_roots``.  A row absent from
    ``data`` is an EMPTY claim and is checked as one: 0 when ``nid`` lies outside that
    root's range, else 6 (shares were withheld).  All rows are verified in one
    rsm_ns_proofs_verify_dev call on GPU ``device``; ``device=None`` runs
    ``NamespaceProof.verify`` per row.  Results never depend on the path."""
    import numpy as np
    ns, nl = int(nmt.namespace_size), 2 * int(nmt.namespace_size) + 32
    if len(row_roots) != width or any(len(r) != nl for r in row_roots) or len(nid) != ns:
        raise RSMError(RSM_EINVAL, "one root of 2 * namespace_size + 32 bytes per row and a namespace of namespace_size bytes")
    proofs = [NamespaceProof(NS_EMPTY, 0, 0, [], None, [], width, nmt, r) for r in range(width)]
    for r, pr in data:
        if not 0 <= r < width or pr.numLeaves != width:
            raise RSMError(RSM_EINVAL, "a proof of a row or a tree that is not the square's")
        proofs[r] = pr
    if device is None:
        out = []
        for r, pr in enumerate(proofs):
            row = NamespaceProof(pr.kind, pr.start, pr.end, pr.nodes, pr.leaf_node, pr.shares, width, nmt, r)
            out.append(row.verify(row_roots[r], nid))
        return out
    sizes = {len(sh) for pr in proofs for sh in pr.shares}
    if len(sizes) > 1:
        raise RSMError(RSM_EINVAL, "shares of different sizes")
    S = sizes.pop() if sizes else 64
    offsets = np.cumsum([0] + [len(pr.shares) for pr in proofs]).astype(np.uint32)
    total = int(offsets[-1])
    packed = b"".join(b"".join(pr.shares) for pr in proofs)
    roots = np.zeros((2, width, nl), np.uint8)  # the rows' roots; no column is asked
    roots[0] = np.frombuffer(b"".join(bytes(r) for r in row_roots), np.uint8).reshape(width, nl)
    recs = b"".join(pr.record() for pr in proofs)
    bufs = [DeviceBuffer(len(recs), device), DeviceBuffer(offsets.nbytes, device), DeviceBuffer(max(total * S, 16), device),
            DeviceBuffer(roots.nbytes, device)]
    try:
        bufs[0].upload(np.frombuffer(recs, np.uint8))
        bufs[1].upload(offsets.view(np.uint8))
        if total:
            bufs[2].upload(np.frombuffer(packed, np.uint8))
        bufs[3].upload(roots.reshape(-1))
        st = verify_namespaces_dev(bufs[0], bufs[1], bufs[2], total, bufs[3], width, S, [(0, Row, r) for r in range(width)],
                                   [bytes(nid)] * width, nmt)
        return [int(x) for x in st]
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# ExtendedDataSquare (extendeddatasquare.go)
# ---------------------------------------------------------------------------
class ExtendedDataSquare:
    def __init__(self, handle: int, codec: Codec, tree_fn, device: int = 0):
        self._h = ctypes.c_void_p(handle)
        self.codec = codec
        self._tree_fn = tree_fn
        self._device = device

    def __del__(self):
        try:
            if self._h:
                library().rsm_eds_free(self._h)
                self._h = None
        except Exception:
            pass

    # --- geometry ---
    def Width(self) -> int:
        return int(library().rsm_eds_width(self._h))

    @property
    def width(self) -> int:
        return self.Width()

    @property
    def originalDataWidth(self) -> int:
        return int(library().rsm_eds_original_width(self._h))

    @property
    def shareSize(self) -> int:
        return int(library().rsm_eds_share_size(self._h))

    # --- cells ---
    def GetCell(self, rowIdx: int, colIdx: int) -> Optional[bytes]:
        buf = ctypes.create_string_buffer(max(self.shareSize, 1))
        rc = library().rsm_eds_get_cell(self._h, rowIdx, colIdx, buf)
        if rc < 0:
            raise _err(rc)
        return buf.raw[: self.shareSize] if rc == 1 else None

    def SetCell(self, rowIdx: int, colIdx: int, newShare: bytes):
        _check(library().rsm_eds_set_cell(self._h, rowIdx, colIdx, newShare, len(newShare)))

    def setCell(self, rowIdx: int, colIdx: int, newShare: Optional[bytes]):
        """Test hook mirroring the reference's unexported setCell (datasquare_test.go:735)."""
        if newShare is None:
            _check(library().rsm_eds_overwrite_cell(self._h, rowIdx, colIdx, None, 0))
        else:
            _check(library().rsm_eds_overwrite_cell(self._h, rowIdx, colIdx, newShare, len(newShare)))

    def Flattened(self) -> List[Optional[bytes]]:
        w, S = self.Width(), self.shareSize
        out = ctypes.create_string_buffer(max(w * w * S, 1))
        pres = ctypes.create_string_buffer(max(w * w, 1))
        _check(library().rsm_eds_flattened(self._h, out, pres))
        raw, p = out.raw, pres.raw
        return [raw[i * S:(i + 1) * S] if p[i] else None for i in range(w * w)]

    def FlattenedODS(self) -> List[Optional[bytes]]:
        f, w, o = self.Flattened(), self.Width(), self.originalDataWidth
        return [f[r * w + c] for r in range(o) for c in range(o)]

    def Row(self, rowIdx: int) -> List[Optional[bytes]]:
        w = self.Width()
        return [self.GetCell(rowIdx, c) for c in range(w)]

    def Col(self, colIdx: int) -> List[Optional[bytes]]:
        w = self.Width()
        return [self.GetCell(r, colIdx) for r in range(w)]

    # --- roots ---
    def _roots(self, axis: int) -> List[bytes]:
        w = self.Width()
        cap = 256
        out = ctypes.create_string_buffer(max(w * cap, 1))
        ln = ctypes.c_uint32(0)
        keep, fn, user = _tree_callback(self._tree_fn)
        _check(library().rsm_eds_roots(self._h, axis, fn, user, out, cap, ctypes.byref(ln)))
        raw = out.raw
        return [raw[i * cap: i * cap + ln.value] for i in range(w)]

    def RowRoots(self) -> List[bytes]:
        return self._roots(Row)

    def ColRoots(self) -> List[bytes]:
        return self._roots(Col)

    def Roots(self) -> List[bytes]:
        return self.RowRoots() + self.ColRoots()

    # --- data root (rsm_eds_data_root) ---
    def DataRoot(self) -> bytes:
        """The 32-byte data root: the RFC 6962 Merkle root over RowRoots() + ColRoots()
        (DataAvailabilityHeader.Hash()).  A complete square with a device context hashes
        its roots and the data root on the GPU; anything else runs the host trees."""
        out = ctypes.create_string_buffer(32)
        keep, fn, user = _tree_callback(self._tree_fn)
        _check(library().rsm_eds_data_root(self._h, fn, user, out))
        return out.raw

    def RootProof(self, axis: int, index: int) -> "RootProof":
        """The proof of RowRoots()[index] (``axis`` = Row) or ColRoots()[index] (Col) under
        DataRoot() (rsm_data_root_prove over this square's roots)."""
        L, w = library(), self.Width()
        roots = self.Roots()
        rec = ctypes.create_string_buffer(max(int(L.rsm_data_root_record_bytes(max(w, 1))), 1))
        _check(L.rsm_data_root_prove(b"".join(roots), w, len(roots[0]) if roots else 0, axis, index, rec))
        return _parse_root_records(rec.raw, [(axis, index)], w)[0]

    # --- Repair (extendeddatacrossword.go:74-84) ---
    def Repair(self, rowRoots: Sequence[bytes], colRoots: Sequence[bytes]) -> None:
        L = library()
        _check(L.rsm_eds_set_context(self._h, device_context(self._device)))
        root_len = len(rowRoots[0]) if rowRoots else 0
        rr = b"".join(bytes(r) for r in rowRoots)
        cr = b"".join(bytes(c) for c in colRoots)
        byz = _Byz()
        keep, fn, user = _tree_callback(self._tree_fn)
        rc = L.rsm_eds_repair(self._h, rr, cr, root_len, fn, user, ctypes.byref(byz))
        if rc == RSM_OK:
            return
        if rc == RSM_EUNREPAIRABLE:
            raise ErrUnrepairableDataSquare
        if rc == RSM_EBYZANTINE:
            w, S = self.Width(), self.shareSize
            out = ctypes.create_string_buffer(max(w * S, 1))
            pres = ctypes.create_string_buffer(max(w, 1))
            _check(L.rsm_eds_byzantine_shares(self._h, out, pres))
            raw, p = out.raw, pres.raw
            raise ErrByzantineData(byz.axis, byz.index, [raw[i * S:(i + 1) * S] if p[i] else None for i in range(w)])
        raise _err(rc)

    # --- share inclusion proofs (rsm_eds_proofs) ---
    def Proofs(self, samples: Sequence[tuple]) -> List["Proof"]:
        """Proofs of ``(axis, index, pos)`` samples (leaf ``pos`` of row / column
        ``index``) against this square's row / column roots, with the tree of the
        square's constructor (NewDefaultTree, the erasured NMT constructor or the
        pool's); other Tree plugins raise RSM_EUNSUPPORTED.  A complete square with a
        device context builds its tree nodes on the GPU once and keeps them until a
        cell changes; anything else runs the host trees."""
        tf = self._tree_fn
        if not (tf is None or tf is NewDefaultTree or isinstance(tf, ErasuredNamespacedMerkleTreeConstructor)):
            raise RSMError(RSM_EUNSUPPORTED, "proofs are built for the DefaultTree and the NMT only")
        keep, fn, user = _tree_callback(tf)
        nmt = tf.params if isinstance(tf, ErasuredNamespacedMerkleTreeConstructor) else None
        L, w, S, n = library(), self.Width(), self.shareSize, len(samples)
        arr = _records(Sample, [(0, a, i, p) for (a, i, p) in samples])
        rb = int(L.rsm_proof_record_bytes(max(w, 1), _nmt_ref(nmt)))
        rec = ctypes.create_string_buffer(max(n * rb, 1))
        sh = ctypes.create_string_buffer(max(n * S, 1))
        _check(L.rsm_eds_proofs(self._h, fn, user, arr, n, rec, sh))
        return _parse_records(rec.raw, sh.raw, samples, w, S, nmt)

    def RowProof(self, rowIdx: int, colIdx: int) -> "Proof":
        """Share (rowIdx, colIdx) with its proof against RowRoots()[rowIdx]
        (computeRowProof, datasquare_test.go:514-537)."""
        return self.Proofs([(Row, rowIdx, colIdx)])[0]

    def ColProof(self, rowIdx: int, colIdx: int) -> "Proof":
        """Share (rowIdx, colIdx) with its proof against ColRoots()[colIdx]."""
        return self.Proofs([(Col, colIdx, rowIdx)])[0]

    def BadEncodingProof(self, axis: int, index: int) -> "BadEncodingProof":
        """The fraud proof a node holding this complete, committed square gives for its row
        (``axis`` = Row) or column ``index``: every share of the vector, each with its proof in
        the orthogonal tree (``Proofs``).  ``.Validate`` decides it against the committed roots."""
        w = self.Width()
        shares = self.Row(index) if axis == Row else self.Col(index)
        if any(s is None for s in shares):
            raise RSMError(RSM_EINVAL, "a fraud proof is built from a complete square")
        return BadEncodingProof(axis, index, shares, self.Proofs([(axis ^ 1, j, index) for j in range(w)]))

    # --- namespace proofs (rsm_eds_namespace_proofs) ---
    def NamespaceProofs(self, nid: bytes, axis: int = 0, indices: Optional[Sequence[int]] = None) -> List["NamespaceProof"]:
        """The shares of namespace ``nid`` in each of rows (``axis`` = Row, the default)
        or columns (Col) ``indices`` (all of them by default), each with the proof that they are all of that vector's
        (nmt's ProveNamespace; verify with ``NamespaceProof.verify`` against
        RowRoots() / ColRoots()).  NMT squares only.  A complete square with a device
        context answers from its cached tree nodes on the GPU; anything else runs the
        host trees."""
        tf = self._tree_fn
        if not isinstance(tf, ErasuredNamespacedMerkleTreeConstructor):
            raise RSMError(RSM_EUNSUPPORTED, "namespace proofs are built for the NMT only")
        keep, fn, user = _tree_callback(tf)
        nmt = tf.params
        if len(nid) != int(nmt.namespace_size):
            raise RSMError(RSM_EINVAL, "a namespace of namespace_size bytes is needed")
        L, w, S = library(), self.Width(), self.shareSize
        indices = list(range(w)) if indices is None else [int(i) for i in indices]
        n = len(indices)
        rb = int(L.rsm_ns_record_bytes(max(w, 1), ctypes.byref(nmt)))
        idx = (ctypes.c_uint32 * max(n, 1))(*indices)
        rec = ctypes.create_string_buffer(max(n * rb, 1))
        offs = (ctypes.c_uint32 * (n + 1))()
        cap = n * w  # a vector has at most w shares of any namespace
        sh = ctypes.create_string_buffer(max(cap * S, 1))
        _check(L.rsm_eds_namespace_proofs(self._h, fn, user, axis, idx, n, bytes(nid), rec, offs, sh, cap))
        return _parse_ns_records(rec.raw, list(offs), sh.raw, indices, w, S, nmt)

    # --- range proofs (rsm_eds_range_proofs) ---
    def RangeProofs(self, queries: Sequence[tuple]) -> List["RangeProof"]:
        """Leaves [start, end) of row / column ``index`` for each ``(axis, index, start,
        end)`` query, with their range proof under that vector's root (nmt's ProveRange;
        verify with ``RangeProof.verify``).  Trees and paths as ``Proofs``."""
        tf = self._tree_fn
        if not (tf is None or tf is NewDefaultTree or isinstance(tf, ErasuredNamespacedMerkleTreeConstructor)):
            raise RSMError(RSM_EUNSUPPORTED, "range proofs are built for the DefaultTree and the NMT only")
        keep, fn, user = _tree_callback(tf)
        nmt = tf.params if isinstance(tf, ErasuredNamespacedMerkleTreeConstructor) else None
        L, w, S, n = library(), self.Width(), self.shareSize, len(queries)
        arr = _records(RangeQuery, [(0, a, i, s, e) for (a, i, s, e) in queries])
        rb = int(L.rsm_range_record_bytes(max(w, 1), _nmt_ref(nmt)))
        cap = sum(max(int(e) - int(s), 0) for (_, _, s, e) in queries)
        rec = ctypes.create_string_buffer(max(n * rb, 1))
        offs = (ctypes.c_uint32 * (n + 1))()
        sh = ctypes.create_string_buffer(max(cap * S, 1))
        _check(L.rsm_eds_range_proofs(self._h, fn, user, arr, n, rec, offs, sh, cap))
        return _parse_range_records(rec.raw, list(offs), sh.raw, queries, w, S, nmt)

    def ShareProof(self, start: int, end: int) -> "ShareProof":
        """ODS shares [start, end) (row-major in the original k x k square) with one
        ``RangeProof`` per touched row and each row root's ``RootProof`` under DataRoot():
        what a rollup or bridge checks against a block header (``.Validate(dataRoot)``)."""
        rows = share_range_queries(self.originalDataWidth, start, end)
        proofs = self.RangeProofs([q[1:] for q in rows])
        roots = self.RowRoots()
        return ShareProof(start, end, proofs, [self.RootProof(Row, q[2]) for q in rows], [roots[q[2]] for q in rows])

    # --- share commitments (rsm_eds_commitments, rsm_eds_subtree_roots) ---
    def _commit(self, start: int, length: int, threshold: int):
        tf = self._tree_fn
        if not isinstance(tf, ErasuredNamespacedMerkleTreeConstructor):
            raise RSMError(RSM_EUNSUPPORTED, "share commitments are built for the NMT only")
        keep, fn, user = _tree_callback(tf)
        m = len(MerkleMountainRangeSizes(length, SubTreeWidth(length, threshold))) if length > 0 and threshold > 0 else 0
        nl = 2 * tf.params.namespace_size + 32
        out, st = ctypes.create_string_buffer(32), (ctypes.c_uint32 * 1)()
        roots, offs = ctypes.create_string_buffer(max(m * nl, 1)), (ctypes.c_uint32 * 2)()
        _check(library().rsm_eds_subtree_roots(self._h, fn, user, _records(BlobRef, [(0, start, length)]), 1, threshold, out,
                                               st, roots, offs))
        if st[0]:
            raise _commit_error(int(st[0]))
        return out.raw, [roots.raw[i * nl:(i + 1) * nl] for i in range(m)]

    def Commitment(self, start: int, length: int, threshold: int = 64) -> bytes:
        """The share commitment of the blob at ODS shares [start, start + length), read off
        the row trees' cached nodes (celestia-app's inclusion.GetCommitment); ``start`` is
        a multiple of ``SubTreeWidth(length, threshold)``.  Equals ``CreateCommitment`` of
        those shares."""
        return self._commit(start, length, threshold)[0]

    def SubtreeRoots(self, start: int, length: int, threshold: int = 64) -> List[bytes]:
        """The blob's subtree roots (min || max || digest each): inner nodes of the row
        trees, the SubtreeRoots of a commitment proof."""
        return self._commit(start, length, threshold)[1]

    def NamespaceData(self, nid: bytes) -> List[tuple]:
        """``(rowIdx, NamespaceProof)`` for every row whose proof for ``nid`` is not
        NS_EMPTY: the answer to celestia-node's GetSharesByNamespace."""
        proofs = self.NamespaceProofs(nid, Row)
        return [(r, pr) for r, pr in enumerate(proofs) if pr.kind != NS_EMPTY]

    def SetCellsVerified(self, rowRoots: Sequence[bytes], colRoots: Sequence[bytes], proofs: Sequence[tuple],
                         device: bool = True) -> List[int]:
        """Verifies sampled shares against the committed roots and sets the cells of
        those that verify (rsm_eds_import_samples).  ``proofs``: ``(axis, index, pos,
        Proof)`` -- the share of cell (index, pos) of a row, (pos, index) of a column.
        Returns one RSM_PROOF_* status per sample: 0 = the cell was set, 4 = verified but
        the cell already had a value, anything else = rejected, nothing written.
        ``device=False`` keeps a context-free square on the host restatement."""
        tf = self._tree_fn
        if not (tf is None or tf is NewDefaultTree or isinstance(tf, ErasuredNamespacedMerkleTreeConstructor)):
            raise RSMError(RSM_EUNSUPPORTED, "samples are verified for the DefaultTree and the NMT only")
        L, n, S = library(), len(proofs), self.shareSize
        if device:
            _check(L.rsm_eds_set_context(self._h, device_context(self._device)))
        keep, fn, user = _tree_callback(tf)
        if any(len(pr.share) != S for (_a, _i, _p, pr) in proofs):
            raise RSMError(RSM_EINVAL, "a sampled share is not of the square's share size")
        arr = _records(Sample, [(0, a, i, p) for (a, i, p, _pr) in proofs])
        shares = b"".join(pr.share for (_a, _i, _p, pr) in proofs)
        records = b"".join(pr.record() for (_a, _i, _p, pr) in proofs)
        status = (ctypes.c_uint32 * max(n, 1))()
        root_len = len(rowRoots[0]) if rowRoots else 0
        rr = b"".join(bytes(r) for r in rowRoots)
        cr = b"".join(bytes(c) for c in colRoots)
        _check(L.rsm_eds_import_samples(self._h, rr, cr, root_len, fn, user, arr, n, shares, records, status, None))
        return [int(status[i]) for i in range(n)]

    def repair_stats(self) -> RepairStats:
        st = RepairStats()
        _check(library().rsm_eds_repair_stats(self._h, ctypes.byref(st)))
        return st

    # --- equality / JSON ---
    def Equals(self, other: "ExtendedDataSquare") -> bool:
        if self.originalDataWidth != other.originalDataWidth:
            return False
        if self.codec.Name() != other.codec.Name():
            return False
        if self.shareSize != other.shareSize or self.Width() != other.Width():
            return False
        return self.Flattened() == other.Flattened()

    def MarshalJSON(self) -> bytes:
        shares = [None if s is None else base64.b64encode(s).decode() for s in self.Flattened()]
        return json.dumps({"data_square": shares, "codec": self.codec.Name()}).encode()

    @staticmethod
    def UnmarshalJSON(b: bytes) -> "ExtendedDataSquare":
        aux = json.loads(b)
        shares = [None if s is None else base64.b64decode(s) for s in aux["data_square"]]
        return ImportExtendedDataSquare(shares, codecs[aux["codec"]], NewDefaultTree)

    def deepCopy(self, codec: Codec) -> "ExtendedDataSquare":
        return ImportExtendedDataSquare(self.Flattened(), codec, self._tree_fn)


def _device_of(codec) -> int:
    return getattr(codec, "device", 0)


def ComputeExtendedDataSquare(data: Sequence[bytes], codec: Codec, treeCreatorFn=NewDefaultTree):
    """extendeddatasquare.go:50-77 on the GPU."""
    keep, ptrs, lens = _bufs(data)
    h = ctypes.c_void_p()
    _check(library().rsm_eds_compute(device_context(_device_of(codec)), ptrs, lens, len(data), ctypes.byref(h)))
    return ExtendedDataSquare(h.value, codec, treeCreatorFn, _device_of(codec))


def ComputeExtendedDataSquareWithBuffer(data: Sequence[bytes], codec: Codec, treeCreator: BufferedTreeConstructor):
    """extendeddatasquare.go:81-92: ComputeExtendedDataSquare with the buffered
    constructor's trees, root parallelism limited to treeCreator.TreeCount()."""
    width = math.isqrt(len(data))
    if width * width < len(data):
        width += 1  # getWidth rounds up (datasquare.go:35-37); the shape check rejects it
    eds = ComputeExtendedDataSquare(data, codec, treeCreator.NewConstructor(width))
    eds.parallelOps = treeCreator.TreeCount()  # setParallelOps
    return eds


def ImportExtendedDataSquare(data: Sequence[Optional[bytes]], codec: Codec, treeCreatorFn=NewDefaultTree):
    """extendeddatasquare.go:95-124 (host-only; no GPU needed until Repair)."""
    keep, ptrs, lens = _bufs(data)
    h = ctypes.c_void_p()
    _check(library().rsm_eds_import(None, ptrs, lens, len(data), ctypes.byref(h)))
    return ExtendedDataSquare(h.value, codec, treeCreatorFn, _device_of(codec))


def NewExtendedDataSquare(codec: Codec, treeCreatorFn, edsWidth: int, shareSize: int):
    """extendeddatasquare.go:129-152 (host-only)."""
    h = ctypes.c_void_p()
    _check(library().rsm_eds_new(None, edsWidth, shareSize, ctypes.byref(h)))
    return ExtendedDataSquare(h.value, codec, treeCreatorFn, _device_of(codec))
