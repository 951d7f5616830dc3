"""ctypes plumbing over lib/libHIPKernel.so's flat C API (include/valign_hip.h).

`Engine` is the device-resident twin of a spawned kernel object: fixed
(read_length, ref_length, scoring), batches passed as device pointers.  torch is used
only to own device memory and streams.  There is no CPU fallback: constructing an
Engine without a gfx950 device raises.
"""
import atexit
import ctypes
import json
import os
import sys
import weakref

from . import build as _build

SW = 0
NW = 1

_lib = None

# Objects that own a handle of the native library.  They are closed by an atexit hook -- while the interpreter, ctypes and
# the HIP runtime are all still whole -- instead of by finalizers that the interpreter's shutdown runs in no particular
# order (a finalizer that frees device memory after the runtime's own teardown ends the process with an abort).
_live = weakref.WeakSet()


def _track(obj):
    _live.add(obj)


def _close_all():
    for obj in list(_live):
        try:
            obj.close()
        except Exception:
            pass


atexit.register(_close_all)


class HipKernelError(RuntimeError):
    pass


class Scoring(ctypes.Structure):
    """Mirror of valign_hip_scoring."""

    _fields_ = [(k, ctypes.c_int32) for k in (
        "match", "mismatch", "gap_read", "gap_ref", "affine",
        "open_read", "ext_read", "open_ref", "ext_ref")]

    @classmethod
    def make(cls, match=2, mismatch=-1, gap_read=-3, gap_ref=-3,
             open_read=None, ext_read=None, open_ref=None, ext_ref=None):
        affine = any(v is not None for v in (open_read, ext_read, open_ref, ext_ref))
        return cls(match, mismatch, gap_read, gap_ref, 1 if affine else 0,
                   gap_read if open_read is None else open_read,
                   gap_read if ext_read is None else ext_read,
                   gap_ref if open_ref is None else open_ref,
                   gap_ref if ext_ref is None else ext_ref)


def plugin_path():
    return _build.HIP_PLUGIN


def lib():
    """Load libHIPKernel.so; raises if it has not been built (never falls back)."""
    global _lib
    if _lib is None:
        path = plugin_path()
        if not os.path.exists(path):
            raise HipKernelError(
                "libHIPKernel.so is missing (%s): run `python -m versalignlib_amd.build`" % path)
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.valign_hip_device_count.restype = ctypes.c_int
        L.valign_hip_engine_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(Scoring), ctypes.c_int, ctypes.c_int,
                                               ctypes.POINTER(vp)]
        L.valign_hip_engine_destroy.restype = None
        L.valign_hip_engine_destroy.argtypes = [vp]
        L.valign_hip_set_traceback_policy.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_band_width.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_band_alignments.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_band_nw.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_band_placed.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_placed_wide.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_extend_wide.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_extend_band.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_extend_zdrop.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_extend_zdrop_rows.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_extend_band_align.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_trace_checkpoints.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_pointer_scratch_cap_mb.argtypes = [vp, ctypes.c_longlong]
        L.valign_hip_set_host_packing.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_half_float_cells.argtypes = [vp, ctypes.c_int]
        L.valign_hip_host_register.argtypes = [vp, ctypes.c_ulonglong]
        L.valign_hip_host_unregister.argtypes = [vp]
        L.valign_hip_set_score_width.argtypes = [vp, ctypes.c_int]
        L.valign_hip_set_ragged_batching.argtypes = [vp, ctypes.c_int]
        L.valign_hip_score_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        L.valign_hip_align_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp, vp]
        L.valign_hip_score_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
        L.valign_hip_align_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int]
        L.valign_hip_align_cigar_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, ctypes.c_int, vp, vp,
                                                    ctypes.c_int, vp]
        L.valign_hip_align_cigar_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp,
                                                  ctypes.c_longlong, vp, vp, ctypes.c_int]
        L.valign_hip_align_span_device.argtypes = L.valign_hip_align_cigar_device.argtypes
        L.valign_hip_align_span_host.argtypes = L.valign_hip_align_cigar_host.argtypes
        L.valign_hip_score_placed_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        L.valign_hip_score_placed_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
        L.valign_hip_score_span_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        L.valign_hip_score_span_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
        L.valign_hip_score_subopt_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, ctypes.c_int, vp, vp]
        L.valign_hip_score_subopt_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int]
        L.valign_hip_score_extend_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        L.valign_hip_score_extend_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int]
        L.valign_hip_align_extend_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                     ctypes.c_int, vp, vp]
        L.valign_hip_align_extend_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                   ctypes.c_longlong, vp, vp, vp, ctypes.c_int]
        L.valign_hip_describe.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p,
                                          ctypes.c_int]
        L.valign_hip_last_error.restype = ctypes.c_char_p
        _lib = L
    return _lib


EXTEND_BAND_BLOCK_ROWS = 8              # VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS
EXTEND_UNREACHED = -(1 << 31)           # VALIGN_HIP_EXTEND_UNREACHED: gscore of a read end the band does not reach

EXPORTED_SYMBOLS = (
    "spawn_alignment_kernel", "set_parameters", "set_logger", "delete_alignment_kernel",
    "valign_hip_device_count", "valign_hip_shard_range", "valign_hip_engine_create", "valign_hip_engine_destroy",
    "valign_hip_set_traceback_policy", "valign_hip_set_pointer_scratch_cap_mb", "valign_hip_set_host_packing", "valign_hip_set_half_float_cells", "valign_hip_host_register", "valign_hip_host_unregister", "valign_hip_set_band_width", "valign_hip_set_band_alignments", "valign_hip_set_band_nw", "valign_hip_set_band_placed", "valign_hip_set_placed_wide", "valign_hip_set_extend_wide", "valign_hip_set_extend_band", "valign_hip_set_extend_band_align", "valign_hip_set_extend_zdrop", "valign_hip_set_extend_zdrop_rows", "valign_hip_set_trace_checkpoints", "valign_hip_set_score_width", "valign_hip_set_ragged_batching", "valign_hip_score_device", "valign_hip_align_device", "valign_hip_score_host", "valign_hip_align_host", "valign_hip_align_cigar_device", "valign_hip_align_cigar_host", "valign_hip_score_placed_device", "valign_hip_score_placed_host", "valign_hip_score_span_device", "valign_hip_score_span_host", "valign_hip_align_span_device", "valign_hip_align_span_host", "valign_hip_score_subopt_device", "valign_hip_score_subopt_host", "valign_hip_score_extend_device", "valign_hip_score_extend_host", "valign_hip_align_extend_device", "valign_hip_align_extend_host", "valign_hip_describe",
    "valign_hip_last_error",
)


def aln_dtype():
    """numpy structured dtype of valign_hip_aln (24 bytes): one record per pair of the compact result format."""
    import numpy as np
    return np.dtype([("read_begin", "<i4"), ("read_end", "<i4"), ("ref_begin", "<i4"), ("ref_end", "<i4"),
                     ("score", "<i4"), ("n_ops", "<u4")])


def placed_dtype():
    """numpy structured dtype of valign_hip_placed (12 bytes): score and half-open end of the best local alignment."""
    import numpy as np
    return np.dtype([("score", "<i4"), ("read_end", "<i4"), ("ref_end", "<i4")])


def subopt_dtype():
    """numpy structured dtype of valign_hip_subopt (20 bytes): the placed record, the runner-up score and where it ends."""
    import numpy as np
    return np.dtype([("score", "<i4"), ("read_end", "<i4"), ("ref_end", "<i4"), ("score2", "<i4"), ("ref_end2", "<i4")])


def extend_dtype():
    """numpy structured dtype of valign_hip_extend (20 bytes): the anchored score and its half-open end cell, the read-end score
    and the half-open reference end that holds it."""
    import numpy as np
    return np.dtype([("score", "<i4"), ("read_end", "<i4"), ("ref_end", "<i4"), ("gscore", "<i4"), ("gref_end", "<i4")])


def span_dtype():
    """numpy structured dtype of valign_hip_span (20 bytes): score and the half-open span of the best local alignment."""
    import numpy as np
    return np.dtype([("score", "<i4"), ("read_begin", "<i4"), ("read_end", "<i4"), ("ref_begin", "<i4"), ("ref_end", "<i4")])


def _err():
    return lib().valign_hip_last_error().decode(errors="replace")


def host_register(array):
    """Page-lock a numpy array for the device (valign_hip_host_register): result buffers registered once take the
    device's copies directly in Engine.align_host(out=...).  Unregister before the array is freed."""
    if lib().valign_hip_host_register(array.ctypes.data, array.nbytes) != 0:
        raise HipKernelError(_err())


def host_unregister(array):
    if lib().valign_hip_host_unregister(array.ctypes.data) != 0:
        raise HipKernelError(_err())


class Engine:
    def __init__(self, read_length, ref_length, scoring=None, device=0, group_lanes=0,
                 rows_per_lane=0):
        self.read_length = int(read_length)
        self.ref_length = int(ref_length)
        self.scoring = scoring or Scoring.make()
        self.device = int(device)
        self._h = ctypes.c_void_p()
        rc = lib().valign_hip_engine_create(self.device, self.read_length, self.ref_length,
                                            ctypes.byref(self.scoring), int(group_lanes),
                                            int(rows_per_lane), ctypes.byref(self._h))
        if rc != 0:
            self._h = None
            raise HipKernelError(_err())
        _track(self)

    def set_traceback_policy(self, policy):
        """0: Default-kernel tie-breaks (default); 1: SSE/AVX-kernel tie-breaks."""
        if lib().valign_hip_set_traceback_policy(self._h, int(policy)) != 0:
            raise HipKernelError(_err())

    def set_pointer_scratch_cap_mb(self, mb):
        """Cap of compute_alignments' device-side pointer scratch in MiB (0: 64 GiB / half the free HBM)."""
        if lib().valign_hip_set_pointer_scratch_cap_mb(self._h, int(mb)) != 0:
            raise HipKernelError(_err())

    def set_host_packing(self, mode):
        """Host-pointer score path: 1 = 4-bit base classes across PCIe (default), 0 = raw ASCII."""
        if lib().valign_hip_set_host_packing(self._h, int(mode)) != 0:
            raise HipKernelError(_err())

    def set_half_float_cells(self, mode):
        """score path: 1 = half-float cells where exact (default), 0 = integer cells only (identical scores)."""
        if lib().valign_hip_set_half_float_cells(self._h, int(mode)) != 0:
            raise HipKernelError(_err())

    def set_score_width(self, bits):
        """0 auto (int16, int32 where needed), 16, or 32."""
        if lib().valign_hip_set_score_width(self._h, int(bits)) != 0:
            raise HipKernelError(_err())

    def set_ragged_batching(self, mode):
        """Length-sorted score batches (classified, packed and swept by length class on the device; host-pointer calls
        and score_device): 0 never (default), 1 when the call is ragged enough, 2 always."""
        if lib().valign_hip_set_ragged_batching(self._h, int(mode)) != 0:
            raise HipKernelError(_err())

    def set_band_width(self, diagonals):
        """> 0: banded Smith-Waterman scores (strip band); 0: every cell."""
        if lib().valign_hip_set_band_width(self._h, int(diagonals)) != 0:
            raise HipKernelError(_err())

    def set_band_alignments(self, on):
        """1: alignments (align_device / align_host) are banded Smith-Waterman alignments on the same block band as the
        scores when band_width > 0; 0 (default): every cell whatever band_width says."""
        if lib().valign_hip_set_band_alignments(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_band_nw(self, on):
        """1: band_width > 0 also applies to NW-variant scores and, with set_band_alignments(1), to NW-variant alignments
        (include/valign_hip.h has the definition); 0 (default): both are refused under a band."""
        if lib().valign_hip_set_band_nw(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_band_placed(self, on):
        """1: with band_width > 0 score_placed_device / score_placed_host return the banded Smith-Waterman score and its first
        in-band end cell from the block chain (describe: ran_placed "chain"; include/valign_hip.h has the definition);
        0 (default): placed scores are refused under a band.  Not read without a band."""
        if lib().valign_hip_set_band_placed(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_placed_wide(self, on):
        """1: unbanded Smith-Waterman score_placed_* / score_span_* calls with score_width = 32, or whose cells can leave int16
        under score_width = 0, run on the pointer-free int32 sweep (describe: ran_placed "wide"; the score does not saturate;
        include/valign_hip.h has the definition); 0 (default): such calls are refused.  Calls inside the int16 range run as
        ever; not read under a band."""
        if lib().valign_hip_set_placed_wide(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_extend_wide(self, on):
        """1: Smith-Waterman-mode score_extend_* calls the int16 register sweep refuses -- score_width = 32, cells that can leave
        int16 under score_width = 0, reads of more than 1024 rows or without a register geometry -- run on the int32 extension sweep
        over 512-row strips (describe: ran_extend "wide"; nothing saturates; include/valign_hip.h has the definition); 0 (default):
        such calls are refused.  Calls the register sweep serves run on it as ever; bands stay refused."""
        if lib().valign_hip_set_extend_wide(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_extend_band(self, on):
        """1: with band_width > 0, score_extend_* calls run banded on the int32 extension sweep: a block band of half-width
        band_width // 2 on the anchor's diagonal, blocks of EXTEND_BAND_BLOCK_ROWS read rows (describe: ran_extend "band"; an
        unreached read end has gscore EXTEND_UNREACHED; include/valign_hip.h has the definition); 0 (default): extension calls are
        refused under a band.  Not read without a band, nor by placed, spanned, suboptimal or alignment calls."""
        if lib().valign_hip_set_extend_band(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_extend_zdrop(self, Z):
        """Z > 0: score_extend_* and align_extend_* calls stop counting rows at the first row that drops -- its maximum lies more
        than Z, less the gap price of its diagonal offset, below the running best -- on the int32 strip sweep (unbanded: ran_extend
        "wide"; under extend_band: "band"; alignments on the banded route only); a dropped pair's read end is EXTEND_UNREACHED, and
        strips below both drops of a wave are skipped (describe: ran_extend_zdrop, extend_zdrop_skipped_waves;
        include/valign_hip.h has the definition).  0 (default): every row counts.  Values outside [0, 2^30] are refused."""
        if not -(1 << 31) <= int(Z) < (1 << 31):
            raise HipKernelError("extend_zdrop must be in [0, 2^30]")
        if lib().valign_hip_set_extend_zdrop(self._h, int(Z)) != 0:
            raise HipKernelError(_err())

    def set_extend_zdrop_rows(self, on):
        """1: under extend_zdrop > 0 and without a band, score_extend_* and align_extend_* calls that would run the int16 register
        sweep without extend_zdrop run its ZDROP instances -- the drop row is decided in the sweep's epilogue from the row maxima it
        already holds (describe: ran_extend / ran_extend_align "rows", ran_extend_zdrop Z, no skipped waves; score_width = 16
        runs; unbanded alignments exist); every other call answers as extend_zdrop alone says, unbanded alignments off the register
        route with a text of their own.  0 (default): as extend_zdrop alone says.  include/valign_hip.h has the definition."""
        if lib().valign_hip_set_extend_zdrop_rows(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_extend_band_align(self, on):
        """1: with band_width > 0 and extend_band = 1, align_extend_* calls run banded on the int32 extension sweep with back
        pointers, whatever the read length (describe: ran_extend_align "band"; an unreached read end is never chosen;
        include/valign_hip.h has the definition); 0 (default): extension alignments are refused under a band.  Not read without a
        band or without extend_band, nor by any other call."""
        if lib().valign_hip_set_extend_band_align(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def set_trace_checkpoints(self, on):
        """1: long-read alignments on the plain row strips keep one boundary row per strip and one strip's pointers, and
        re-fill strip after strip along the walk (identical results, a scratch that grows with R + F instead of R x F);
        0 (default): every pointer of every strip.  Other paths run as ever (describe: ran_align_fill)."""
        if lib().valign_hip_set_trace_checkpoints(self._h, int(on)) != 0:
            raise HipKernelError(_err())

    def score_device(self, opt, reads, refs, scores=None, stream=None):
        """reads/refs: torch uint8 CUDA tensors [n, R] / [n, F]; -> int16 CUDA tensor [n].

        Asynchronous on torch's current stream (or `stream`)."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if scores is None:
            scores = torch.empty(n, dtype=torch.int16, device=reads.device)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_score_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(),
                                           scores.data_ptr(), st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return scores

    def align_device(self, opt, reads, refs, rows=None, idx=None, stream=None):
        """-> rows uint8 CUDA [n, 2, R+F], idx int16 CUDA [n, 4] (async on the current stream)."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        AL = self.read_length + self.ref_length
        if rows is None:
            rows = torch.empty((n, 2, AL), dtype=torch.uint8, device=reads.device)
        if idx is None:
            idx = torch.empty((n, 4), dtype=torch.int16, device=reads.device)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_align_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(),
                                           rows.data_ptr(), idx.data_ptr(), st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return rows, idx

    def score_host(self, opt, reads, refs, threads=1):
        """Host-pointer path of score_alignments without the plugin object: reads/refs are C-contiguous
        numpy uint8 arrays [n, R] / [n, F]; the library gets one pointer per sequence."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8
        assert reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        scores = np.zeros(n, dtype=np.int16)
        rc = lib().valign_hip_score_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data,
                                         scores.ctypes.data, int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return scores

    def align_host(self, opt, reads, refs, threads=1, out=None):
        """Host-pointer path of compute_alignments into contiguous numpy buffers (no operator new[] blocks):
        -> rows uint8 [n, 2, R+F], idx int16 [n, 4].  `out` = (rows, idx) of an earlier call is written in place
        (a caller that loops keeps its result buffers, like any FFI binding would)."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        AL = self.read_length + self.ref_length
        if out is not None:
            rows, idx = out
            assert rows.shape == (n, 2, AL) and rows.dtype == np.uint8 and rows.flags.c_contiguous
            assert idx.shape == (n, 4) and idx.dtype == np.int16 and idx.flags.c_contiguous
        else:
            rows = np.zeros((n, 2, AL), dtype=np.uint8)
            idx = np.zeros((n, 4), dtype=np.int16)
        rc = lib().valign_hip_align_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, rows.ctypes.data,
                                         idx.ctypes.data, int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return rows, idx

    def align_cigar_device(self, opt, reads, refs, extended=False, ops_stride=64, stream=None, out=None):
        """Placed CIGARs without the rows: -> recs int32 CUDA [n, 6] (read_begin, read_end, ref_begin, ref_end, score,
        n_ops -- `recs.cpu().numpy().view(aln_dtype())` names them) and ops int32 CUDA [n, ops_stride] (length << 4 | BAM
        code; a pair stores its first min(n_ops, ops_stride) ops, the rest of its row is not written).  Asynchronous on
        the current stream (or `stream`).  `out` = (recs, ops) of an earlier call is written in place."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is not None:
            recs, ops = out
            assert recs.is_cuda and recs.is_contiguous() and recs.dtype == torch.int32 and tuple(recs.shape) == (n, 6)
            assert ops.is_cuda and ops.is_contiguous() and ops.dtype == torch.int32 and tuple(ops.shape) == (n, int(ops_stride))
        else:
            recs = torch.empty((n, 6), dtype=torch.int32, device=reads.device)
            ops = torch.empty((n, int(ops_stride)), dtype=torch.int32, device=reads.device)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_align_cigar_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(),
                                                 1 if extended else 0, recs.data_ptr(), ops.data_ptr(), int(ops_stride),
                                                 st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return recs, ops

    def _packed_host(self, call, opt, reads, refs, extended, threads, ops_cap, before=(), after=()):
        """What the three *_host calls of the compact format share: the pointer arrays, `ops` sized from a guess (`ops_cap`,
        default 16 per pair) and the single retry with the exact size.  `call` is the library's entry point; `before` and
        `after` are the arguments it takes in front of `extended` (an int here) and behind `ops_needed`.  -> recs, ops, offsets."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        recs = np.zeros(n, dtype=aln_dtype())
        offsets = np.zeros(n + 1, dtype=np.int64)
        cap = 16 * n if ops_cap is None else int(ops_cap)
        for _ in range(2):
            ops = np.zeros(max(cap, 1), dtype=np.uint32)
            needed = ctypes.c_longlong(0)
            rc = call(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, *before, extended, recs.ctypes.data,
                      ops.ctypes.data, cap, offsets.ctypes.data, ctypes.byref(needed), *after, int(threads))
            if rc == 0:
                return recs, ops[:int(offsets[n])], offsets
            if needed.value <= cap:
                break
            cap = needed.value
        raise HipKernelError(_err())

    def align_cigar_host(self, opt, reads, refs, extended=False, threads=1, ops_cap=None):
        """Host-pointer path of the compact result format: -> recs (structured, aln_dtype()) [n], ops uint32
        [offsets[n]], offsets int64 [n + 1]; pair p's ops are ops[offsets[p]:offsets[p + 1]].  `ops` is sized from a guess
        (`ops_cap`, default 16 per pair) and the call repeated once with the exact size where that was too small."""
        return self._packed_host(lib().valign_hip_align_cigar_host, opt, reads, refs, 1 if extended else 0, threads, ops_cap)

    def score_placed_device(self, opt, reads, refs, out=None, stream=None):
        """Placed Smith-Waterman scores: -> int32 CUDA [n, 3] (score, read_end, ref_end -- `out.cpu().numpy().view(
        placed_dtype())[:, 0]` names them).  Asynchronous on the current stream (or `stream`); `out` of an earlier call is
        written in place.  opt 1, bands, traceback_policy 1 and int32 cells are refused (HipKernelError)."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is None:
            out = torch.empty((n, 3), dtype=torch.int32, device=reads.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and tuple(out.shape) == (n, 3)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_score_placed_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), out.data_ptr(),
                                                  st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return out

    def score_placed_host(self, opt, reads, refs, threads=1):
        """Host-pointer path of the placed scores: numpy uint8 [n, R] / [n, F] -> structured array [n] (placed_dtype())."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        placed = np.zeros(n, dtype=placed_dtype())
        rc = lib().valign_hip_score_placed_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, placed.ctypes.data,
                                                int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return placed

    def score_span_device(self, opt, reads, refs, out=None, stream=None):
        """Spanned Smith-Waterman scores: -> int32 CUDA [n, 5] (score, read_begin, read_end, ref_begin, ref_end --
        `out.cpu().numpy().view(span_dtype())[:, 0]` names them).  Asynchronous on the current stream (or `stream`); `out` of
        an earlier call is written in place.  Refused (HipKernelError) where placed scores are, and under any band."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is None:
            out = torch.empty((n, 5), dtype=torch.int32, device=reads.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and tuple(out.shape) == (n, 5)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_score_span_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), out.data_ptr(),
                                                st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return out

    def score_span_host(self, opt, reads, refs, threads=1):
        """Host-pointer path of the spanned scores: numpy uint8 [n, R] / [n, F] -> structured array [n] (span_dtype())."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        spans = np.zeros(n, dtype=span_dtype())
        rc = lib().valign_hip_score_span_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, spans.ctypes.data,
                                              int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return spans

    def align_span_device(self, opt, reads, refs, extended=False, ops_stride=64, stream=None, out=None):
        """Spanned CIGARs: the alignment of every pair's span, filled and walked on the span's window instead of the whole
        matrix (include/valign_hip.h has the definition).  -> recs int32 CUDA [n, 6] and ops int32 CUDA [n, ops_stride], as
        align_cigar_device returns them; the coordinates are score_span_device's, the score score_placed_device's.
        Asynchronous on the current stream (or `stream`).  `out` = (recs, ops) of an earlier call is written in place.
        Refused (HipKernelError) where spanned scores are."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.is_contiguous() and refs.is_contiguous()
        assert reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is not None:
            recs, ops = out
            assert recs.is_cuda and recs.is_contiguous() and recs.dtype == torch.int32 and tuple(recs.shape) == (n, 6)
            assert ops.is_cuda and ops.is_contiguous() and ops.dtype == torch.int32 and tuple(ops.shape) == (n, max(int(ops_stride), 1))
        else:
            recs = torch.empty((n, 6), dtype=torch.int32, device=reads.device)
            ops = torch.empty((n, max(int(ops_stride), 1)), dtype=torch.int32, device=reads.device)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_align_span_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), int(extended),
                                                recs.data_ptr(), ops.data_ptr(), int(ops_stride), st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return recs, ops

    def align_span_host(self, opt, reads, refs, extended=False, threads=1, ops_cap=None):
        """Host-pointer path of the spanned CIGARs: -> recs (structured, aln_dtype()) [n], ops uint32 [offsets[n]], offsets
        int64 [n + 1], as align_cigar_host returns them.  `ops` is sized from a guess (`ops_cap`, default 16 per pair) and the
        call repeated once with the exact size where that was too small."""
        return self._packed_host(lib().valign_hip_align_span_host, opt, reads, refs, int(extended), threads, ops_cap)

    def score_subopt_device(self, opt, reads, refs, mask, out=None, stream=None):
        """Suboptimal Smith-Waterman scores: -> int32 CUDA [n, 5] (score, read_end, ref_end, score2, ref_end2 --
        `out.cpu().numpy().view(subopt_dtype())[:, 0]` names them): the placed record plus the largest column maximum at
        more than `mask` columns from the end cell and the smallest column that holds it (include/valign_hip.h has the
        definition).  Asynchronous on the current stream (or `stream`); `out` of an earlier call is written in place.
        Refused (HipKernelError) for mask < 0, where unbanded placed scores are, under any band and on the row strips."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is None:
            out = torch.empty((n, 5), dtype=torch.int32, device=reads.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and tuple(out.shape) == (n, 5)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_score_subopt_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), int(mask),
                                                  out.data_ptr(), st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return out

    def score_subopt_host(self, opt, reads, refs, mask, threads=1):
        """Host-pointer path of the suboptimal scores: numpy uint8 [n, R] / [n, F] -> structured array [n] (subopt_dtype())."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        subopt = np.zeros(n, dtype=subopt_dtype())
        rc = lib().valign_hip_score_subopt_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, int(mask),
                                                subopt.ctypes.data, int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return subopt

    def score_extend_device(self, opt, reads, refs, out=None, stream=None):
        """Extension scores: -> int32 CUDA [n, 5] (score, read_end, ref_end, gscore, gref_end --
        `out.cpu().numpy().view(extend_dtype())[:, 0]` names them): the best score of an alignment that starts before read[0]
        and ref[0] with the cell it ends in, and the best score that consumes the read to its last ACGT base with the smallest
        reference end that holds it (include/valign_hip.h has the definition).  Asynchronous on the current stream (or
        `stream`); `out` of an earlier call is written in place.  Refused (HipKernelError) for opt & 0xF == 1,
        traceback_policy = 1, any band, score_width = 32, cells that could leave int16 and on the row strips."""
        import torch
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        n = reads.shape[0]
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is None:
            out = torch.empty((n, 5), dtype=torch.int32, device=reads.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.int32 and tuple(out.shape) == (n, 5)
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_score_extend_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), out.data_ptr(), st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return out

    def score_extend_host(self, opt, reads, refs, threads=1):
        """Host-pointer path of the extension scores: numpy uint8 [n, R] / [n, F] -> structured array [n] (extend_dtype())."""
        import numpy as np
        n = reads.shape[0]
        assert reads.dtype == np.uint8 and refs.dtype == np.uint8 and reads.flags.c_contiguous and refs.flags.c_contiguous
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.read_length)).astype(np.uint64)
        fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(self.ref_length)).astype(np.uint64)
        extend = np.zeros(n, dtype=extend_dtype())
        rc = lib().valign_hip_score_extend_host(self._h, int(opt), n, rp.ctypes.data, fp.ctypes.data, extend.ctypes.data, int(threads))
        if rc != 0:
            raise HipKernelError(_err())
        return extend

    def align_extend_device(self, opt, reads, refs, end_bonus=-1, extended=False, ops_stride=64, with_extend=True, stream=None, out=None):
        """Extension alignments: -> recs int32 CUDA [n, 6], ops int32 CUDA [n, ops_stride] (the layout of align_cigar_device)
        and, with_extend, the extension records int32 CUDA [n, 5] (else None): per pair the alignment from the anchor before
        read[0] and ref[0] to the best cell (end_bonus < 0) or, where gscore + end_bonus >= score, to the read end
        (include/valign_hip.h has the definition).  Asynchronous on the current stream (or `stream`); `out` = (recs, ops,
        extend) of an earlier call is written in place.  Refused (HipKernelError) where score_extend_device is, and on the
        int32 route of extend_wide."""
        import torch
        n = reads.shape[0]
        assert reads.is_cuda and refs.is_cuda and reads.dtype == torch.uint8 and refs.dtype == torch.uint8
        assert reads.is_contiguous() and refs.is_contiguous()
        assert tuple(reads.shape) == (n, self.read_length) and tuple(refs.shape) == (n, self.ref_length)
        if out is not None:
            recs, ops, extend = out
        else:
            recs = torch.empty((n, 6), dtype=torch.int32, device=reads.device)
            ops = torch.empty((n, int(ops_stride)), dtype=torch.int32, device=reads.device)
            extend = torch.empty((n, 5), dtype=torch.int32, device=reads.device) if with_extend else None
        assert recs.is_cuda and recs.is_contiguous() and recs.dtype == torch.int32 and tuple(recs.shape) == (n, 6)
        assert ops.is_cuda and ops.is_contiguous() and ops.dtype == torch.int32 and tuple(ops.shape) == (n, int(ops_stride))
        assert extend is None or (extend.is_cuda and extend.is_contiguous() and extend.dtype == torch.int32 and tuple(extend.shape) == (n, 5))
        st = stream if stream is not None else torch.cuda.current_stream(reads.device)
        rc = lib().valign_hip_align_extend_device(self._h, int(opt), n, reads.data_ptr(), refs.data_ptr(), int(end_bonus),
                                                  1 if extended else 0, recs.data_ptr(), ops.data_ptr(), int(ops_stride),
                                                  extend.data_ptr() if extend is not None else None, st.cuda_stream)
        if rc != 0:
            raise HipKernelError(_err())
        return recs, ops, extend

    def align_extend_host(self, opt, reads, refs, end_bonus=-1, extended=False, with_extend=True, threads=1, ops_cap=None):
        """Host-pointer path of the extension alignments: -> recs (structured, aln_dtype()) [n], ops uint32 [offsets[n]],
        offsets int64 [n + 1] as align_cigar_host returns them, and the extension records (structured, extend_dtype()) [n]
        with_extend (else None).  `ops` is sized from a guess (`ops_cap`, default 16 per pair) and the call repeated once
        with the exact size where that was too small."""
        import numpy as np
        extend = np.zeros(reads.shape[0], dtype=extend_dtype()) if with_extend else None
        return self._packed_host(lib().valign_hip_align_extend_host, opt, reads, refs, 1 if extended else 0, threads, ops_cap, before=(int(end_bonus),),
                                 after=(extend.ctypes.data if extend is not None else None,)) + (extend,)

    def describe(self, opt=0, n=0):
        buf = ctypes.create_string_buffer(8192)
        lib().valign_hip_describe(self._h, int(opt), int(n), buf, len(buf))
        return json.loads(buf.value.decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().valign_hip_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        if sys is None or sys.is_finalizing():      # interpreter shutdown: the atexit hook has closed what was open
            return
        try:
            self.close()
        except Exception:
            pass
