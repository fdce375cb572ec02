"""Host-side mirror of the reference's lib-crate API over the C ABI (include/circkit.h).

    circkit::lmsr_index(&[u8]) -> usize      lib/src/canonicalize.rs:5    -> lmsr_index(b)
    circkit::lmsr(&[u8]) -> Vec<u8>          lib/src/canonicalize.rs:41   -> lmsr(b)
    circkit::canonicalize(&[u8]) -> Vec<u8>  lib/src/canonicalize.rs:54   -> canonicalize(b)
    xxhash_rust::xxh3::xxh3_64               call site src/uniq.rs:45     -> xxh3_64(b)
    Monomerizer::last_monomer_end_index[_sensitive]  lib/src/monomerize.rs:97, :122  -> monomer_end_index(b, ...)
    Monomerizer::monomerize[_sensitive]      lib/src/monomerize.rs:138, :146 -> monomerize(b, ...)
    the worker + writer closures             src/monomerize.rs:72-131        -> monomers_batch(data, offsets, ...)
    one shard of `circkit uniq`              src/uniq.rs:27-66               -> uniq_batch(data, offsets, ...)

Everything computes on the GPU through libcirckit_hip.so; there is no CPU fallback -- importing works
without a GPU (so the ABI can be inspected), creating a Context does not.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CIRCKIT_LIB: another build of the same library (tools/build_variant.sh: A/B timing, the poison-check build of tests/) --
# selected here instead of being copied over the in-tree file, which build.py's mtime check would then take for current
LIB_PATH = os.environ.get("CIRCKIT_LIB") or os.path.join(_HERE, "libcirckit_hip.so")

OK = 0
ERRORS = {-1: "INVALID_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "TOO_LONG", -5: "OOM", -6: "NOT_ASCII"}

# every symbol include/circkit.h declares, with ctypes signatures
_vp, _u64, _u32, _i, _sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "circkit_ctx_create": (_i, [_i, ctypes.POINTER(_vp)]),
    "circkit_ctx_destroy": (_i, [_vp]),
    "circkit_last_error": (ctypes.c_char_p, [_vp]),
    "circkit_ctx_set_stream": (_i, [_vp, _vp]),
    "circkit_ctx_use_own_stream": (_i, [_vp]),
    "circkit_ctx_synchronize": (_i, [_vp]),
    "circkit_ctx_last_kernel_ms": (_i, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "circkit_ctx_batch_status": (_i, [_vp, ctypes.POINTER(_u32)]),
    "circkit_ctx_set_long_record_scratch": (_i, [_vp, _u64]),
    "circkit_ctx_last_batch_mode": (_i, [_vp, ctypes.POINTER(_u32)]),
    "circkit_canonicalize_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "circkit_lmsr_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "circkit_xxh3_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "circkit_canonicalize_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "circkit_host_alloc": (_vp, [_sz]),
    "circkit_host_free": (None, [_vp]),
    "circkit_lmsr_index": (_i, [_vp, _vp, _sz, ctypes.POINTER(_sz)]),
    "circkit_lmsr": (_i, [_vp, _vp, _sz, _vp]),
    "circkit_canonicalize": (_i, [_vp, _vp, _sz, _vp]),
    "circkit_xxh3_64": (_i, [_vp, _vp, _sz, ctypes.POINTER(_u64)]),
    "circkit_uniq_reset": (_i, [_vp, _u64]),
    "circkit_uniq_insert_device": (_i, [_vp, _vp, _u64, _u64]),
    "circkit_uniq_insert_pairs_device": (_i, [_vp, _vp, _vp, _u64]),
    "circkit_uniq_partition_device": (_i, [_vp, _vp, _u64, _u64, ctypes.c_uint32, _vp, _vp, _vp]),
    "circkit_uniq_insert_rows_device": (_i, [_vp, _vp, _u64]),
    "circkit_uniq_lookup_rows_device": (_i, [_vp, _vp, _u64, _vp]),
    "circkit_uniq_gather_device": (_i, [_vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "circkit_uniq_lookup_device": (_i, [_vp, _vp, _u64, _vp]),
    "circkit_uniq_status": (_i, [_vp, ctypes.POINTER(_u32)]),
    "circkit_uniq_resolve_device": (_i, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "circkit_uniq_first_seen": (_i, [_vp, _vp, _u64, _u64, _vp]),
    "circkit_uniq_compact_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "circkit_uniq_compact_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "circkit_uniq_batch": (_i, [_vp, _vp, _vp, _u64, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(_u64)]),
    "circkit_fasta_parse": (_i, [_vp, _sz, _i, _i, ctypes.POINTER(_vp), ctypes.POINTER(_sz)]),
    "circkit_fasta_error": (ctypes.c_char_p, [_vp]),
    "circkit_fasta_n_records": (_u64, [_vp]),
    "circkit_fasta_bytes": (_vp, [_vp]),
    "circkit_fasta_offsets": (_vp, [_vp]),
    "circkit_fasta_record": (_i, [_vp, _u64] + [ctypes.POINTER(_sz)] * 4),
    "circkit_fasta_free": (None, [_vp]),
    "circkit_fasta_parse_device": (_i, [_vp, _vp, _u64, _i, _i, _vp, _u64, _vp, _u64, _vp, _vp]),
    "circkit_fasta_parse_status": (_i, [_vp] + [ctypes.POINTER(_u64)] * 3),
    "circkit_fasta_parse_text": (_i, [_vp, _vp, _u64, _i, _i, _vp, _u64, _vp, _u64, _vp, _vp] + [ctypes.POINTER(_u64)] * 3),
    "circkit_fasta_write_device": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "circkit_fasta_write_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "circkit_fasta_write_text": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, _vp, ctypes.POINTER(_u64)]),
    "circkit_synth_fill_device": (_i, [_vp, _u64, _u64, _u64, _vp]),
    "circkit_fixed_offsets_device": (_i, [_vp, _u64, _u64, _u64, _vp]),
    "circkit_bench_copy_device": (_i, [_vp, _vp, _vp, _u64, _u32]),
    "circkit_normalize": (_sz, [_vp, _sz, _vp, ctypes.POINTER(_i)]),
    "circkit_orfs_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64]),
    "circkit_orfs_status": (_i, [_vp, ctypes.POINTER(_u64)]),
    "circkit_orfs_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, ctypes.POINTER(_u64)]),
    "circkit_find_orfs": (_i, [_vp, _vp, _sz, _vp, _sz, ctypes.POINTER(_sz)]),
    "circkit_monomerize_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "circkit_monomerize_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "circkit_monomer_end_index": (_i, [_vp, _vp, _sz, _vp, ctypes.POINTER(_sz), ctypes.POINTER(_i)]),
    "circkit_monomers_compact_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "circkit_monomers_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "circkit_monomers_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(_u64)]),
    "circkit_windows_gather_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "circkit_windows_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "circkit_windows_of_records_device": (_i, [_vp, _vp, _u64, _u32, ctypes.c_int64, ctypes.c_double, _vp]),
    "circkit_orfs_windows_device": (_i, [_vp, _vp, _vp, _u64, _u64, _i, _vp]),
    "circkit_windows_gather": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, ctypes.POINTER(_u64)]),
    "circkit_windows_translate_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "circkit_translate_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "circkit_windows_translate": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64)]),
    "circkit_sketch_batch_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "circkit_sketch_status": (_i, [_vp, ctypes.POINTER(_u64), ctypes.POINTER(_u32)]),
    "circkit_sketch_compare_device": (_i, [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _u64, _vp]),
    "circkit_sketch_compare_status": (_i, [_vp, ctypes.POINTER(_u64)]),
    "circkit_sketch_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "circkit_sketch_compare": (_i, [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _u64, _vp]),
    "circkit_cluster_candidates_device": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64]),
    "circkit_cluster_candidates_status": (_i, [_vp, ctypes.POINTER(_u64)]),
    "circkit_cluster_link_device": (_i, [_vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "circkit_cluster_link_status": (_i, [_vp] + [ctypes.POINTER(_u64)] * 3),
    "circkit_cluster_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, ctypes.POINTER(_u64)]),
    "circkit_sketch_anchors_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "circkit_prealign_pairs_device": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "circkit_prealign_status": (_i, [_vp] + [ctypes.POINTER(_u64)] * 2),
    "circkit_prealign_pairs_of_labels_device": (_i, [_vp, _vp, _u64, _vp]),
    "circkit_prealign_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp]),
    "circkit_distance_pairs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "circkit_distance_status": (_i, [_vp] + [ctypes.POINTER(_u64)] * 2),
    "circkit_distance_pairs": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "circkit_version": (ctypes.c_char_p, []),
}

# circkit_orf / circkit_orf_params (include/circkit.h)
ORF_NO_STOP = 0xFFFFFFFF
ORF_DTYPE = np.dtype([("length", "<u8"), ("start", "<u4"), ("stop", "<u4"), ("wraps", "<u4"), ("strand", "<u4")])
# circkit_window (include/circkit.h)
WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])
# circkit_fasta_span (include/circkit.h)
FASTA_SPAN_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8")])
WINDOW_KINDS = {"rotate_bases": 0, "rotate_percent": 1, "cat": 2, "decat": 3, "revcomp": 4}


# NCBI genetic codes as "AAs" lines: residue of codon c0 c1 c2 at 16*c0 + 4*c1 + c2 with T, C, A, G = 0..3
_STANDARD_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
GENETIC_CODES = {1: _STANDARD_CODE, 4: _STANDARD_CODE[:14] + "W" + _STANDARD_CODE[15:], 11: _STANDARD_CODE}


# circkit_translate_params (include/circkit.h)
class TranslateParams(ctypes.Structure):
    _fields_ = [("aa", ctypes.c_uint8 * 64), ("unknown", ctypes.c_uint8), ("first_as_m", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 6)]


def translate_params(table=1, unknown="X", first_as_m=False):
    """circkit_translate_params from Python values.  table: a key of GENETIC_CODES or 64 characters / bytes in the order of an
    NCBI "AAs" line; unknown: the residue of a codon with a byte outside ACGT; first_as_m: write the first residue of a window
    whose first codon is three ACGT symbols as 'M'."""
    aa = table if isinstance(table, (str, bytes, bytearray)) else GENETIC_CODES[int(table)]
    aa = aa.encode("latin-1") if isinstance(aa, str) else bytes(aa)
    unk = unknown.encode("latin-1") if isinstance(unknown, str) else bytes(unknown)
    if len(aa) != 64 or len(unk) != 1:
        raise ValueError("a genetic code has 64 residues and `unknown` is one")
    p = TranslateParams()
    for k, v in enumerate(aa):
        p.aa[k] = v
    p.unknown, p.first_as_m = unk[0], int(bool(first_as_m))
    return p


# circkit_sketch_params / CIRCKIT_SKETCH_EMPTY (include/circkit.h)
SKETCH_EMPTY = 0xFFFFFFFFFFFFFFFF


class SketchParams(ctypes.Structure):
    _fields_ = [("k", _u32), ("log2_bins", _u32), ("seed", _u64), ("reserved", _u32 * 2)]


def sketch_params(k=21, log2_bins=8, seed=0):
    """circkit_sketch_params from Python values: k-mers of k symbols (4 .. 32), 1 << log2_bins bins (log2_bins 4 .. 10), the seed
    xor-ed into every canonical k-mer before it is hashed.  The library checks the ranges."""
    p = SketchParams()
    p.k, p.log2_bins, p.seed = int(k), int(log2_bins), int(seed) & SKETCH_EMPTY
    return p


# circkit_cluster_params (include/circkit.h)
class ClusterParams(ctypes.Structure):
    _fields_ = [("n_bands", _u32), ("band_bins", _u32), ("min_similarity_q16", _u32), ("min_filled", _u32), ("reserved", _u32 * 2)]


def cluster_params(n_bands=64, band_bins=2, min_similarity=0.2, min_filled=8):
    """circkit_cluster_params from Python values: n_bands (1 .. 64) bands of band_bins (1 .. 16) bins each make the candidate
    pairs; a scored pair links when filled >= min_filled and match / filled >= min_similarity (0 .. 1, kept as the nearest
    multiple of 2^-16).  The library checks the ranges."""
    p = ClusterParams()
    q = int(round(float(min_similarity) * 65536))
    p.n_bands, p.band_bins, p.min_filled = int(n_bands), int(band_bins), int(min_filled)
    p.min_similarity_q16 = q if 0 <= q < 2 ** 32 else 2 ** 32 - 1
    return p


# circkit_prealign_params / CIRCKIT_ANCHOR_NONE (include/circkit.h)
ANCHOR_NONE = 0xFFFFFFFF


class PrealignParams(ctypes.Structure):
    _fields_ = [("k", _u32), ("log2_bins", _u32), ("min_votes", _u32), ("reserved", _u32)]


def prealign_params(k=21, log2_bins=8, min_votes=4):
    """circkit_prealign_params from Python values: the k and log2_bins the sketch and its anchors were made with; a pair is
    aligned when at least min_votes (>= 1) shared bins agree on one rotation and strand.  The library checks the ranges."""
    p = PrealignParams()
    p.k, p.log2_bins, p.min_votes = int(k), int(log2_bins), int(min_votes)
    return p


# circkit_distance_params / CIRCKIT_DISTANCE_OVER / CIRCKIT_DISTANCE_MAX (include/circkit.h)
DISTANCE_OVER = 0xFFFFFFFF
DISTANCE_MAX = 255


class DistanceParams(ctypes.Structure):
    _fields_ = [("max_distance", _u32), ("reserved", _u32 * 3)]


def distance_params(max_distance=32):
    """circkit_distance_params from Python values: a pair's distance is reported when it is at most max_distance (0 .. 255) and
    as DISTANCE_OVER otherwise.  The library checks the range."""
    p = DistanceParams()
    p.max_distance = int(max_distance) & 0xFFFFFFFF
    return p


class OrfParams(ctypes.Structure):
    _fields_ = [("start_codons", (ctypes.c_uint8 * 3) * 64), ("n_start_codons", _u32),
                ("stop_codons", (ctypes.c_uint8 * 3) * 64), ("n_stop_codons", _u32),
                ("min_length", _u64), ("min_ratio", ctypes.c_double), ("min_wraps", _u32), ("max_wraps", _u32),
                ("require_stop", _u32), ("strands", _u32), ("mode", _u32)]


STRANDS = {"forward": 1, "reverse": 2, "both": 3}


def orf_params(start_codons=("ATG",), stop_codons=("TAA", "TAG", "TGA"), min_length=0, min_ratio=0.0, min_wraps=0, max_wraps=3,
               require_stop=False, strands="both", mode="longest"):
    """circkit_orf_params from Python values.  Codons are str/bytes; one whose length is not 3 never matches (the
    reference compares &str) and is left out.  strands: "forward" | "reverse" | "both" or a bit mask; mode: "longest"
    (per stop, the CLI) or "all" (find order)."""
    p = OrfParams()
    for field, codons in (("start", start_codons), ("stop", stop_codons)):
        cs = [c.encode() if isinstance(c, str) else bytes(c) for c in codons]
        cs = [c for c in cs if len(c) == 3]
        if len(cs) > 64:
            raise ValueError("at most 64 %s codons" % field)
        arr = getattr(p, field + "_codons")
        for k, c in enumerate(cs):
            for j in range(3):
                arr[k][j] = c[j]
        setattr(p, "n_%s_codons" % field, len(cs))
    p.min_length, p.min_ratio = int(min_length), float(min_ratio)
    p.min_wraps, p.max_wraps, p.require_stop = int(min_wraps), int(max_wraps), int(bool(require_stop))
    p.strands = STRANDS[strands] if isinstance(strands, str) else int(strands)
    p.mode = {"longest": 0, "all": 1}[mode] if isinstance(mode, str) else int(mode)
    return p


def _orf_arrays(offsets, orfs):
    return {"offsets": offsets, "start": orfs["start"].copy(), "stop": orfs["stop"].copy(), "length": orfs["length"].copy(),
            "wraps": orfs["wraps"].copy(), "strand": orfs["strand"].copy()}


# circkit_monomerize_params (include/circkit.h)
MONOMER_NONE = 0xFFFFFFFF
BOTH_CUTOFFS = ("Both overlap_dist and overlap_min_identity are set. They are mutually exclusive since they may produce "
                "conflicting filtering results.")


class MonomerizeParams(ctypes.Structure):
    _fields_ = [("seed_len", _u32), ("use_identity", _u32), ("overlap_dist", _u64), ("min_identity", ctypes.c_double),
                ("sensitive", _u32)]


def monomerize_params(seed_len=10, max_mismatch=None, min_identity=None, sensitive=False):
    """circkit_monomerize_params from Python values (MonomerizerBuilder: lib/src/monomerize.rs:19-41).  Setting both
    cut-offs raises ValueError with the builder's message; neither = no mismatch allowed.  The seed length and the identity
    are checked by the library (CIRCKIT_ERR_INVALID_ARG)."""
    if max_mismatch is not None and min_identity is not None:
        raise ValueError(BOTH_CUTOFFS)
    p = MonomerizeParams()
    p.seed_len = int(seed_len) if 0 <= int(seed_len) < 2 ** 32 else 0
    p.use_identity = int(min_identity is not None)
    p.overlap_dist = int(max_mismatch or 0)
    p.min_identity = float(min_identity) if min_identity is not None else 0.0
    p.sensitive = int(bool(sensitive))
    return p


# circkit_monomer_filter (include/circkit.h)
class MonomerFilter(ctypes.Structure):
    _fields_ = [("min_length", _u64), ("max_length", _u64), ("min_overlap", _u64), ("min_overlap_percent", ctypes.c_double),
                ("use_min_overlap_percent", _u32), ("keep_all", _u32)]


def monomer_filter(min_length=0, max_length=None, min_overlap=None, min_overlap_percent=None, keep_all=False):
    """circkit_monomer_filter from Python values: the writer's options of `circkit monomerize` (src/monomerize.rs:94-131).
    None = the option is not given."""
    f = MonomerFilter()
    f.min_length = int(min_length)
    f.max_length = 2 ** 64 - 1 if max_length is None else int(max_length)
    f.min_overlap = int(min_overlap or 0)
    f.use_min_overlap_percent = int(min_overlap_percent is not None)
    f.min_overlap_percent = float(min_overlap_percent) if min_overlap_percent is not None else 0.0
    f.keep_all = int(bool(keep_all))
    return f


_lib = None


class CirckitError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("circkit error %s (%d): %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code


def load_library():
    """Loads the HIP shared library; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Loading
        # torch first makes our NEEDED libamdhip64.so.7 bind to that copy instead of pulling in /opt/rocm's
        # as a second runtime (two runtimes in one process cannot both own the GPU).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)      # AttributeError here = header/library mismatch
            except AttributeError:
                if os.environ.get("CIRCKIT_LIB"):    # an explicitly chosen variant (e.g. an older round's build in an A/B run) may lack newer symbols
                    import warnings
                    warnings.warn("CIRCKIT_LIB=%s lacks %s (a stale variant build?): calls of it will fail" % (LIB_PATH, name))
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _ptr(x):
    """Device or host address of a torch tensor / numpy array / None."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return x.ctypes.data


class Context:
    """One GPU's worth of the hot path (circkit_ctx)."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = _vp()
        rc = self._lib.circkit_ctx_create(int(device), ctypes.byref(h))
        self._h = h
        if rc != OK:
            msg = self._lib.circkit_last_error(h).decode() if h else "no usable HIP device %d" % device
            if h:
                self._lib.circkit_ctx_destroy(h)
                self._h = None
            raise CirckitError(rc, msg)
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.circkit_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise CirckitError(rc, self._lib.circkit_last_error(self._h).decode())

    # -- stream / timing ------------------------------------------------------------------------
    def set_stream(self, stream_handle):
        """Run on this hipStream_t (int handle; 0/None = HIP's default stream), e.g.
        torch.cuda.current_stream().cuda_stream so the work is ordered with torch's."""
        self._check(self._lib.circkit_ctx_set_stream(self._h, stream_handle or None))

    def use_own_stream(self):
        self._check(self._lib.circkit_ctx_use_own_stream(self._h))

    def synchronize(self):
        self._check(self._lib.circkit_ctx_synchronize(self._h))

    def last_kernel_ms(self):
        ms = ctypes.c_float(0)
        self._check(self._lib.circkit_ctx_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def batch_status(self):
        n = _u32(0)
        rc = self._lib.circkit_ctx_batch_status(self._h, ctypes.byref(n))
        if rc not in (OK, -4):
            self._check(rc)
        return n.value

    def set_long_record_scratch(self, nbytes):
        self._check(self._lib.circkit_ctx_set_long_record_scratch(self._h, int(nbytes)))

    def last_batch_mode(self):
        m = _u32(0)
        self._check(self._lib.circkit_ctx_last_batch_mode(self._h, ctypes.byref(m)))
        return m.value

    # -- device-resident batches (torch tensors on this ctx's GPU) -------------------------------
    def canonicalize_batch_device(self, d_bytes, d_offsets, n_records, out_bytes=None, out_index=None,
                                  out_strand=None, out_xxh3=None):
        self._check(self._lib.circkit_canonicalize_batch_device(
            self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), _ptr(out_bytes), _ptr(out_index),
            _ptr(out_strand), _ptr(out_xxh3)))

    def lmsr_batch_device(self, d_bytes, d_offsets, n_records, out_bytes=None, out_index=None):
        self._check(self._lib.circkit_lmsr_batch_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records),
                                                        _ptr(out_bytes), _ptr(out_index)))

    def xxh3_batch_device(self, d_bytes, d_offsets, n_records, out_hash):
        self._check(self._lib.circkit_xxh3_batch_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records),
                                                        _ptr(out_hash)))

    def synth_fill_device(self, seed, first_base, n_bases, d_bytes):
        self._check(self._lib.circkit_synth_fill_device(self._h, int(seed), int(first_base), int(n_bases), _ptr(d_bytes)))

    def fixed_offsets_device(self, base, record_len, n_records, d_offsets):
        self._check(self._lib.circkit_fixed_offsets_device(self._h, int(base), int(record_len), int(n_records),
                                                           _ptr(d_offsets)))

    def bench_copy_device(self, d_src, d_dst, nbytes, variant=0):
        self._check(self._lib.circkit_bench_copy_device(self._h, _ptr(d_src), _ptr(d_dst), int(nbytes), int(variant)))

    def uniq_reset(self, expected_keys):
        self._check(self._lib.circkit_uniq_reset(self._h, int(expected_keys)))

    def uniq_insert_device(self, d_hash, n, base_index=0):
        self._check(self._lib.circkit_uniq_insert_device(self._h, _ptr(d_hash), int(n), int(base_index)))

    def uniq_insert_pairs_device(self, d_hash, d_index, n):
        self._check(self._lib.circkit_uniq_insert_pairs_device(self._h, _ptr(d_hash), _ptr(d_index), int(n)))

    def uniq_partition_device(self, d_hash, n, base_index, world, d_rows, d_counts, d_slot):
        self._check(self._lib.circkit_uniq_partition_device(self._h, _ptr(d_hash), int(n), int(base_index), int(world), _ptr(d_rows),
                                                            _ptr(d_counts), _ptr(d_slot)))

    def uniq_insert_rows_device(self, d_rows, n):
        self._check(self._lib.circkit_uniq_insert_rows_device(self._h, _ptr(d_rows), int(n)))

    def uniq_lookup_rows_device(self, d_rows, n, d_answers):
        self._check(self._lib.circkit_uniq_lookup_rows_device(self._h, _ptr(d_rows), int(n), _ptr(d_answers)))

    def uniq_gather_device(self, d_answers, d_slot, n, base_index, d_first_seen, d_keep=None):
        self._check(self._lib.circkit_uniq_gather_device(self._h, _ptr(d_answers), _ptr(d_slot), int(n), int(base_index), _ptr(d_first_seen),
                                                         _ptr(d_keep)))

    def uniq_lookup_device(self, d_hash, n, d_first_seen):
        self._check(self._lib.circkit_uniq_lookup_device(self._h, _ptr(d_hash), int(n), _ptr(d_first_seen)))

    def uniq_resolve_device(self, d_hash, n, base_index, d_first_seen, d_keep=None):
        self._check(self._lib.circkit_uniq_resolve_device(self._h, _ptr(d_hash), int(n), int(base_index), _ptr(d_first_seen), _ptr(d_keep)))

    def uniq_first_seen(self, hashes, base_index=0):
        """Host-buffer streaming form (the CLI's batch loop): folds the batch into the ctx table, grown on demand, and
        returns first_seen (numpy uint64)."""
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        out = np.empty(max(len(hashes), 1), dtype=np.uint64)
        self._check(self._lib.circkit_uniq_first_seen(self._h, _ptr(hashes), len(hashes), int(base_index), _ptr(out)))
        return out[:len(hashes)]

    def uniq_status(self):
        """Waits for the queued table work; raises CirckitError (OOM) if keys found no slot."""
        self._check(self._lib.circkit_uniq_status(self._h, None))

    def uniq_overflowed(self):
        """Waits like uniq_status; returns how many inserted records found no slot for their key (0: the table took them all)
        instead of raising for an overflow.  Lookups answer ~0 for such keys until the next uniq_reset."""
        n = _u32(0)
        rc = self._lib.circkit_uniq_status(self._h, ctypes.byref(n))
        if rc != OK and not (rc == -5 and n.value):
            self._check(rc)
        return n.value

    def uniq_compact_device(self, d_bytes, d_offsets, n_records, d_first_seen, d_out_bytes, d_out_offsets, d_out_src, base_index=0,
                            d_dup_src=None, d_dup_first=None):
        """Enqueues circkit_uniq_compact_device: the records with d_first_seen[i] == base_index + i packed into the CSR batch
        d_out_bytes / d_out_offsets, d_out_src[j] = the input index of output record j; the others listed in d_dup_src (their
        input index) and d_dup_first (their d_first_seen, a global index), each where given.  uniq_compact_status() waits and
        returns the totals; uniq_status() says whether the table behind d_first_seen took every key."""
        self._check(self._lib.circkit_uniq_compact_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), _ptr(d_first_seen),
                                                          int(base_index), _ptr(d_out_bytes), _ptr(d_out_offsets), _ptr(d_out_src),
                                                          _ptr(d_dup_src), _ptr(d_dup_first)))

    def uniq_compact_status(self):
        """Waits for the last uniq compact; returns (number of kept records, their bytes)."""
        m, b = _u64(0), _u64(0)
        self._check(self._lib.circkit_uniq_compact_status(self._h, ctypes.byref(m), ctypes.byref(b)))
        return m.value, b.value

    def uniq_batch(self, data, offsets, canonicalize=False):
        """What `circkit uniq` (`-c` with canonicalize=True) writes for a host CSR batch of normalized records, as a CSR batch:
        (out_data, out_offsets, out_src, first_seen).  out_src[j] = the input index of output record j; first_seen[i] = the
        index of the first record with record i's canonical hash: record i is a duplicate of it where that is not i."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty(max(len(data), 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        out_src = np.zeros(max(n, 1), dtype=np.uint64)
        fs = np.zeros(max(n, 1), dtype=np.uint64)
        m = _u64(0)
        self._check(self._lib.circkit_uniq_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, int(bool(canonicalize)),
                                                 _ptr(out), _ptr(out_off), _ptr(out_src), _ptr(fs), ctypes.byref(m)))
        m = m.value
        return out[:int(out_off[m])], out_off[:m + 1], out_src[:m], fs[:n]

    # -- host batches (numpy) -------------------------------------------------------------------
    def canonicalize_batch(self, data, offsets, want_bytes=True, want_index=False, want_strand=False,
                           want_xxh3=False):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.empty(max(len(data), 1), dtype=np.uint8) if want_bytes else None
        idx = np.empty(max(n, 1), dtype=np.uint32) if want_index else None
        st = np.empty(max(n, 1), dtype=np.uint8) if want_strand else None
        hs = np.empty(max(n, 1), dtype=np.uint64) if want_xxh3 else None
        self._check(self._lib.circkit_canonicalize_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n,
                                                         _ptr(out), _ptr(idx), _ptr(st), _ptr(hs)))
        return {"bytes": out[:len(data)] if out is not None else None,
                "index": idx[:n] if idx is not None else None,
                "strand": st[:n] if st is not None else None,
                "xxh3": hs[:n] if hs is not None else None}

    # -- circular ORFs ---------------------------------------------------------------------------
    def orfs_batch_device(self, d_bytes, d_offsets, n_records, d_orf_offsets, d_orfs, capacity, params=None, **kw):
        """Enqueues circkit_orfs_batch_device.  d_orfs: a device buffer of `capacity` 24-byte descriptors (ORF_DTYPE);
        orfs_status() waits and returns the total."""
        p = params if params is not None else orf_params(**kw)
        self._check(self._lib.circkit_orfs_batch_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), ctypes.byref(p),
                                                        _ptr(d_orf_offsets), _ptr(d_orfs), int(capacity)))

    def orfs_status(self):
        """Waits for the last orfs_batch_device; returns its total, raises CirckitError (OOM) beyond the capacity."""
        t = _u64(0)
        self._check(self._lib.circkit_orfs_status(self._h, ctypes.byref(t)))
        return t.value

    def orfs_batch(self, data, offsets, **params):
        """ORFs of every record of a host CSR batch of normalized records (see orf_params for the keywords).  Returns numpy
        arrays: offsets (n + 1; record i's ORFs are [offsets[i], offsets[i+1]), forward before reverse), start, stop
        (ORF_NO_STOP = None), length, wraps, strand (0 forward, 1 reverse)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        p = orf_params(**params)
        orf_off = np.zeros(n + 1, dtype=np.uint64)
        cap = max(n, 1) * 4
        while True:
            orfs = np.zeros(cap, dtype=ORF_DTYPE)
            total = _u64(0)
            rc = self._lib.circkit_orfs_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, ctypes.byref(p),
                                              _ptr(orf_off), _ptr(orfs), cap, ctypes.byref(total))
            if rc == -5 and total.value > cap:           # grow to the reported total and run again
                cap = total.value
                continue
            self._check(rc)
            return _orf_arrays(orf_off, orfs[:total.value])

    def find_orfs(self, s):
        """lib/src/orfs.rs:41 find_orfs: [(start, stop or None, wraps, length)] in the reference's order."""
        s = bytes(s)
        buf = ctypes.create_string_buffer(s, max(len(s), 1))
        cap = max(len(s), 1)
        while True:
            out = np.zeros(cap, dtype=ORF_DTYPE)
            cnt = _sz(0)
            rc = self._lib.circkit_find_orfs(self._h, ctypes.addressof(buf), len(s), _ptr(out), cap, ctypes.byref(cnt))
            if rc == -5 and cnt.value > cap:
                cap = cnt.value
                continue
            self._check(rc)
            return [(int(o["start"]), None if int(o["stop"]) == ORF_NO_STOP else int(o["stop"]), int(o["wraps"]), int(o["length"]))
                    for o in out[:cnt.value]]

    # -- FASTA text on the device ------------------------------------------------------------------
    def fasta_parse_device(self, d_text, n_text, d_out_bytes, byte_capacity, d_out_offsets, record_capacity, d_head=None, d_raw=None,
                           first_chunk=True, final_chunk=True):
        """Enqueues circkit_fasta_parse_device: the text d_text[0, n_text) (device) becomes the CSR batch d_out_bytes /
        d_out_offsets (uint64[record_capacity + 1]); d_head / d_raw (FASTA_SPAN_DTYPE[record_capacity], device) receive the header
        and raw sequence spans when given.  fasta_parse_status() waits and returns the counts."""
        self._check(self._lib.circkit_fasta_parse_device(self._h, _ptr(d_text), int(n_text), int(bool(first_chunk)), int(bool(final_chunk)),
                                                         _ptr(d_out_bytes), int(byte_capacity), _ptr(d_out_offsets), int(record_capacity),
                                                         _ptr(d_head), _ptr(d_raw)))

    def fasta_parse_status(self):
        """Waits for the last device parse; returns (records, payload bytes, consumed).  Raises CirckitError: OOM when the
        records or the payload exceeded the capacities (nothing was written; the message has the true counts), INVALID_ARG on the
        format error or when the payload buffer overlapped the text."""
        r, b, used = _u64(0), _u64(0), _u64(0)
        self._check(self._lib.circkit_fasta_parse_status(self._h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(used)))
        return r.value, b.value, used.value

    def fasta_parse_text(self, text, first_chunk=True, final_chunk=True, keep_on_device=False):
        """fasta_parse on the device: FASTA text -> (records, normalized_bytes, offsets, consumed), records = [(head, raw_seq)].
        One copy in, the parse on the device, one copy home (circkit_fasta_parse_text).  keep_on_device: the bytes and the offsets
        stay on the device and are returned as torch tensors (uint8 / int64 holding the uint64 offsets); only the spans come home.
        Raises ValueError on a format error, as fasta_parse does."""
        text = bytes(text)
        n = len(text)
        cap_r = (n + 1) // 2
        if keep_on_device:
            import torch
            dev = torch.device("cuda", self.device)
            with torch.cuda.device(dev):
                d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)).to(dev)
                d_out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
                d_off = torch.empty(cap_r + 1, dtype=torch.int64, device=dev)
                d_spans = torch.empty((2, max(cap_r, 1), 2), dtype=torch.int64, device=dev)
                self.fasta_parse_device(d_text, n, d_out, n, d_off, cap_r, d_spans[0], d_spans[1], first_chunk=first_chunk, final_chunk=final_chunk)
                r, b, used = _u64(0), _u64(0), _u64(0)
                rc = self._lib.circkit_fasta_parse_status(self._h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(used))
                if rc != OK:
                    msg = self._lib.circkit_last_error(self._h).decode()
                    if msg.startswith("FASTA parse error"):
                        raise ValueError(msg)
                    raise CirckitError(rc, msg)
                spans = d_spans[:, :r.value].cpu().numpy().view(np.uint64)
                data, offs = d_out[:b.value], d_off[:r.value + 1]
                head, raw = spans[0], spans[1]
        else:
            buf = np.frombuffer(text, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
            data = np.empty(max(n, 1), dtype=np.uint8)
            offs = np.zeros(cap_r + 1, dtype=np.uint64)
            head = np.zeros((max(cap_r, 1), 2), dtype=np.uint64)
            raw = np.zeros((max(cap_r, 1), 2), dtype=np.uint64)
            r, b, used = _u64(0), _u64(0), _u64(0)
            rc = self._lib.circkit_fasta_parse_text(self._h, _ptr(buf), n, int(bool(first_chunk)), int(bool(final_chunk)), _ptr(data), n, _ptr(offs),
                                                    cap_r, _ptr(head), _ptr(raw), ctypes.byref(r), ctypes.byref(b), ctypes.byref(used))
            if rc != OK:
                msg = self._lib.circkit_last_error(self._h).decode()
                if msg.startswith("FASTA parse error"):
                    raise ValueError(msg)
                raise CirckitError(rc, msg)
            data, offs = data[:b.value].copy(), offs[:r.value + 1].copy()
        recs = [(text[int(head[i][0]):int(head[i][0] + head[i][1])], text[int(raw[i][0]):int(raw[i][0] + raw[i][1])]) for i in range(r.value)]
        return recs, data, offs, used.value

    # -- FASTA text from the device ------------------------------------------------------------------
    def fasta_write_device(self, d_text, n_text, d_head, n_heads, n_out, d_out_text, out_capacity, d_out_offsets, d_body=None,
                           d_body_offsets=None, d_raw=None, d_src=None, n_src=None, d_labels=None):
        """Enqueues circkit_fasta_write_device: output record k = '>' head label '\\n' body '\\n' into
        d_out_text[d_out_offsets[k] .. d_out_offsets[k + 1]).  d_head / d_raw: the spans of fasta_parse_device; d_src (n_src
        entries): a compact's d_out_src; d_labels: the windows of orfs_windows_device; the body is d_body / d_body_offsets (a CSR
        batch of n_out records) or the raw spans.  fasta_write_status() waits and returns the totals."""
        self._check(self._lib.circkit_fasta_write_device(self._h, _ptr(d_text), int(n_text), _ptr(d_head), _ptr(d_raw), int(n_heads), _ptr(d_src),
                                                         int(n_heads if n_src is None else n_src), _ptr(d_labels), _ptr(d_body), _ptr(d_body_offsets),
                                                         int(n_out), _ptr(d_out_text), int(out_capacity), _ptr(d_out_offsets)))

    def fasta_write_status(self):
        """Waits for the last FASTA write; returns (total bytes, invalid records).  Raises CirckitError: OOM when the total
        exceeded the capacity, INVALID_ARG when the output overlapped an input or records were invalid."""
        t, bad = _u64(0), _u64(0)
        self._check(self._lib.circkit_fasta_write_status(self._h, ctypes.byref(t), ctypes.byref(bad)))
        return t.value, bad.value

    def fasta_write_text(self, text, head, body=None, offsets=None, raw=None, src=None, labels=None):
        """FASTA text of host arrays, written on the device (circkit_fasta_write_text): (bytes, out_offsets).  text: the input
        text the spans point into; head / raw: (R, 2) uint64 arrays of (off, len) or FASTA_SPAN_DTYPE; body / offsets: a CSR
        batch, one record per output; src: the kept-record map; labels: an array of WINDOW_DTYPE.  Exactly one of body (with
        offsets) and raw.  Grows its buffer to the reported total and runs again; invalid records raise CirckitError."""
        text = bytes(text)
        buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, dtype=np.uint8)
        head = np.ascontiguousarray(head).view(np.uint64).reshape(-1, 2)
        n_heads = len(head)
        if (body is None) != (offsets is None) or (body is None) == (raw is None):
            raise ValueError("exactly one of body (with offsets) and raw must be given")
        if raw is not None:
            raw = np.ascontiguousarray(raw).view(np.uint64).reshape(-1, 2)
            if len(raw) != n_heads:
                raise ValueError("head and raw must have one span per record each")
        if src is not None:
            src = np.ascontiguousarray(src, dtype=np.uint64)
        n_src = n_heads if src is None else len(src)
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=WINDOW_DTYPE)
        if body is not None:
            body = np.ascontiguousarray(body, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            if len(offsets) < 1 or int(offsets[-1]) > len(body):
                raise ValueError("offsets must end inside body")
            if not len(body):
                body = np.zeros(1, dtype=np.uint8)
        n_out = len(offsets) - 1 if offsets is not None else len(labels) if labels is not None else n_src
        if labels is not None and len(labels) != n_out:
            raise ValueError("one label per output record")
        out_off = np.zeros(n_out + 1, dtype=np.uint64)
        cap = max(len(text) + (len(body) if body is not None else 0), 1)
        while True:
            out = np.empty(cap, dtype=np.uint8)
            total = _u64(0)
            rc = self._lib.circkit_fasta_write_text(self._h, _ptr(buf) if text else None, len(text), _ptr(head) if n_heads else None,
                                                    _ptr(raw) if raw is not None else None, n_heads, _ptr(src) if src is not None else None, n_src,
                                                    _ptr(labels) if labels is not None else None, _ptr(body), _ptr(offsets), n_out, _ptr(out), cap,
                                                    _ptr(out_off), ctypes.byref(total))
            if rc == -5 and cap < total.value < 2 ** 64 - 1:      # grow to the reported total and run again
                cap = total.value
                continue
            self._check(rc)
            return out[:total.value].tobytes(), out_off

    # -- cyclic windows ------------------------------------------------------------------------
    def windows_gather_device(self, d_bytes, d_offsets, n_records, d_windows, n_windows, d_out_bytes, out_capacity, d_out_offsets):
        """Enqueues circkit_windows_gather_device: window k of d_windows (WINDOW_DTYPE, device) packed into
        d_out_bytes[d_out_offsets[k] .. d_out_offsets[k + 1]).  windows_status() waits and returns the totals."""
        self._check(self._lib.circkit_windows_gather_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), _ptr(d_windows),
                                                            int(n_windows), _ptr(d_out_bytes), int(out_capacity), _ptr(d_out_offsets)))

    def windows_status(self):
        """Waits for the last windows gather; returns (total bytes, invalid windows).  Raises CirckitError: OOM when the total
        exceeded the capacity, INVALID_ARG when the output overlapped the payload or windows were invalid."""
        t, bad = _u64(0), _u64(0)
        self._check(self._lib.circkit_windows_status(self._h, ctypes.byref(t), ctypes.byref(bad)))
        return t.value, bad.value

    def windows_of_records_device(self, d_offsets, n_records, kind, d_windows, bases=0, percent=0.0):
        """Enqueues circkit_windows_of_records_device: one window per record into d_windows (WINDOW_DTYPE, device).  kind: a key
        of WINDOW_KINDS or its number; bases / percent are read by the two rotate kinds only."""
        k = WINDOW_KINDS[kind] if isinstance(kind, str) else int(kind)
        self._check(self._lib.circkit_windows_of_records_device(self._h, _ptr(d_offsets), int(n_records), k, int(bases), float(percent),
                                                                _ptr(d_windows)))

    def orfs_windows_device(self, d_orf_offsets, d_orfs, n_records, n_orfs, d_windows, include_stop=False):
        """Enqueues circkit_orfs_windows_device: one window per ORF of an orfs_batch_device result into d_windows."""
        self._check(self._lib.circkit_orfs_windows_device(self._h, _ptr(d_orf_offsets), _ptr(d_orfs), int(n_records), int(n_orfs),
                                                          int(bool(include_stop)), _ptr(d_windows)))

    def windows_gather(self, data, offsets, windows):
        """The windows' bytes of a host CSR batch, packed: (out_bytes, out_offsets).  windows: an array of WINDOW_DTYPE.  Grows
        its buffer to the reported total and runs again, as orfs_batch does; invalid windows raise CirckitError."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        windows = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
        n, m = len(offsets) - 1, len(windows)
        out_off = np.zeros(m + 1, dtype=np.uint64)
        cap = max(len(data), 1)
        while True:
            out = np.empty(cap, dtype=np.uint8)
            total = _u64(0)
            rc = self._lib.circkit_windows_gather(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(windows) if m else None,
                                                  m, _ptr(out), cap, _ptr(out_off), ctypes.byref(total))
            if rc == -5 and cap < total.value < 2 ** 64 - 1:      # grow to the reported total and run again
                cap = total.value
                continue
            self._check(rc)
            return out[:total.value], out_off

    # -- proteins of cyclic windows ---------------------------------------------------------------
    def windows_translate_device(self, d_bytes, d_offsets, n_records, d_windows, n_windows, d_out_aa, out_capacity, d_out_offsets,
                                 params=None, **kw):
        """Enqueues circkit_windows_translate_device: the protein of window k of d_windows (WINDOW_DTYPE, device) packed into
        d_out_aa[d_out_offsets[k] .. d_out_offsets[k + 1]).  params: a translate_params() result, or its keywords.
        translate_status() waits and returns the totals."""
        p = params if params is not None else translate_params(**kw)
        self._check(self._lib.circkit_windows_translate_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), _ptr(d_windows),
                                                               int(n_windows), ctypes.byref(p), _ptr(d_out_aa), int(out_capacity),
                                                               _ptr(d_out_offsets)))

    def translate_status(self):
        """Waits for the last translate; returns (total residues, invalid windows).  Raises CirckitError as windows_status does."""
        t, bad = _u64(0), _u64(0)
        self._check(self._lib.circkit_translate_status(self._h, ctypes.byref(t), ctypes.byref(bad)))
        return t.value, bad.value

    def windows_translate(self, data, offsets, windows, params=None, capacity=None, **kw):
        """The windows' proteins of a host CSR batch, packed: (aa_bytes, aa_offsets).  windows: an array of WINDOW_DTYPE; params or
        the keywords of translate_params.  Grows its buffer (capacity: its first size) to the reported total and runs again, as
        windows_gather does; invalid windows raise CirckitError."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        windows = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
        p = params if params is not None else translate_params(**kw)
        n, m = len(offsets) - 1, len(windows)
        out_off = np.zeros(m + 1, dtype=np.uint64)
        cap = max(len(data) // 3, 1) if capacity is None else max(int(capacity), 1)
        while True:
            out = np.empty(cap, dtype=np.uint8)
            total = _u64(0)
            rc = self._lib.circkit_windows_translate(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, _ptr(windows) if m else None,
                                                     m, ctypes.byref(p), _ptr(out), cap, _ptr(out_off), ctypes.byref(total))
            if rc == -5 and cap < total.value < 2 ** 64 - 1:      # grow to the reported total and run again
                cap = total.value
                continue
            self._check(rc)
            return out[:total.value], out_off

    # -- sketches of circular records ---------------------------------------------------------------
    def sketch_batch_device(self, d_bytes, d_offsets, n_records, d_out_sketch, d_out_n_kmers=None, params=None, **kw):
        """Enqueues circkit_sketch_batch_device: row i of d_out_sketch (uint64[n_records << log2_bins], device) = the cyclic k-mer
        MinHash sketch of record i, d_out_n_kmers[i] (uint32, optional) its valid k-mers.  params: a sketch_params() result, or
        its keywords.  sketch_status() waits and returns the totals."""
        p = params if params is not None else sketch_params(**kw)
        self._check(self._lib.circkit_sketch_batch_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), ctypes.byref(p),
                                                          _ptr(d_out_sketch), _ptr(d_out_n_kmers)))

    def sketch_status(self):
        """Waits for the last sketch; returns (valid k-mers of all records, records of 2^31 symbols or more).  Raises CirckitError
        (TOO_LONG) when the latter is not 0."""
        t, bad = _u64(0), _u32(0)
        self._check(self._lib.circkit_sketch_status(self._h, ctypes.byref(t), ctypes.byref(bad)))
        return t.value, bad.value

    def sketch_compare_device(self, d_sketch_a, n_a, d_sketch_b, n_b, log2_bins, d_pairs, n_pairs, d_out):
        """Enqueues circkit_sketch_compare_device: d_out[2p], d_out[2p + 1] = (match, filled) of row d_pairs[2p] of d_sketch_a and
        row d_pairs[2p + 1] of d_sketch_b (uint32, device).  sketch_compare_status() waits."""
        self._check(self._lib.circkit_sketch_compare_device(self._h, _ptr(d_sketch_a), int(n_a), _ptr(d_sketch_b), int(n_b), int(log2_bins),
                                                            _ptr(d_pairs), int(n_pairs), _ptr(d_out)))

    def sketch_compare_status(self):
        """Waits for the last compare; returns its invalid pairs (0), or raises CirckitError (INVALID_ARG) when there were any."""
        bad = _u64(0)
        self._check(self._lib.circkit_sketch_compare_status(self._h, ctypes.byref(bad)))
        return bad.value

    def sketch_batch(self, data, offsets, params=None, **kw):
        """The sketches of a host CSR batch: (rows, n_kmers) with rows an (n, 1 << log2_bins) uint64 array.  params or the keywords
        of sketch_params."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = params if params is not None else sketch_params(**kw)
        n = len(offsets) - 1
        bins = 1 << p.log2_bins if 0 <= p.log2_bins < 32 else 1
        rows = np.empty((n, bins), dtype=np.uint64)
        counts = np.empty(n, dtype=np.uint32)
        self._check(self._lib.circkit_sketch_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, ctypes.byref(p),
                                                   _ptr(rows) if n else None, _ptr(counts) if n else None))
        return rows, counts

    def sketch_compare(self, sk_a, sk_b, pairs):
        """(match, filled) of every pair (i, j): row i of sk_a against row j of sk_b, host arrays of one bin count.  sk_b may be
        sk_a itself.  Invalid pairs raise CirckitError after the valid ones were computed."""
        same = sk_b is sk_a
        sk_a = np.ascontiguousarray(sk_a, dtype=np.uint64)
        sk_b = sk_a if same else np.ascontiguousarray(sk_b, dtype=np.uint64)
        if sk_a.ndim != 2 or sk_b.ndim != 2 or sk_a.shape[1] != sk_b.shape[1] or sk_a.shape[1] & (sk_a.shape[1] - 1) or not sk_a.shape[1]:
            raise ValueError("sketches are (n, bins) arrays of one power-of-two bin count")
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        m = len(pairs)
        out = np.zeros((m, 2), dtype=np.uint32)
        self._check(self._lib.circkit_sketch_compare(self._h, _ptr(sk_a), len(sk_a), _ptr(sk_b), len(sk_b), sk_a.shape[1].bit_length() - 1,
                                                     _ptr(pairs) if m else None, m, _ptr(out) if m else None))
        return out[:, 0].copy(), out[:, 1].copy()

    # -- clusters of circular records ----------------------------------------------------------------
    def cluster_candidates_device(self, d_sketch, n_records, log2_bins, d_pair_offsets, d_pairs, capacity, params=None, **kw):
        """Enqueues circkit_cluster_candidates_device: the candidate pairs of the sketch rows d_sketch as a CSR by the later
        record, d_pair_offsets (uint64[n_records + 1]) and d_pairs (uint32[2 * capacity]), the layout sketch_compare_device
        takes.  params: a cluster_params() result, or its keywords.  cluster_candidates_status() waits and returns the total."""
        p = params if params is not None else cluster_params(**kw)
        self._check(self._lib.circkit_cluster_candidates_device(self._h, _ptr(d_sketch), int(n_records), int(log2_bins), ctypes.byref(p),
                                                                _ptr(d_pair_offsets), _ptr(d_pairs), int(capacity)))

    def cluster_candidates_status(self):
        """Waits for the last candidates call; returns the number of pairs.  Raises CirckitError (OOM) when they exceeded the
        capacity: the message has the number."""
        t = _u64(0)
        self._check(self._lib.circkit_cluster_candidates_status(self._h, ctypes.byref(t)))
        return t.value

    def cluster_link_device(self, n_records, d_pairs, d_scores, n_pairs, d_labels, params=None, **kw):
        """Enqueues circkit_cluster_link_device: single linkage over the pairs whose (match, filled) in d_scores pass the
        threshold; d_labels[i] (uint64, device) = the smallest record of i's cluster.  cluster_link_status() waits."""
        p = params if params is not None else cluster_params(**kw)
        self._check(self._lib.circkit_cluster_link_device(self._h, int(n_records), _ptr(d_pairs), _ptr(d_scores), int(n_pairs), ctypes.byref(p),
                                                          _ptr(d_labels)))

    def cluster_link_status(self):
        """Waits for the last link; returns (clusters, linked pairs, invalid pairs).  Raises CirckitError (INVALID_ARG) when
        pairs were invalid."""
        a, b, bad = _u64(0), _u64(0), _u64(0)
        self._check(self._lib.circkit_cluster_link_status(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(bad)))
        return a.value, b.value, bad.value

    def cluster_batch(self, data, offsets, k=21, log2_bins=8, seed=0, params=None, **kw):
        """The clusters of a host CSR batch: (labels, n_clusters); labels[i] = the smallest record of record i's cluster.  params
        or the keywords of cluster_params."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        p = params if params is not None else cluster_params(**kw)
        sp = sketch_params(k=k, log2_bins=log2_bins, seed=seed)
        n = len(offsets) - 1
        labels = np.empty(n, dtype=np.uint64)
        m = _u64(0)
        self._check(self._lib.circkit_cluster_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, ctypes.byref(sp), ctypes.byref(p),
                                                    _ptr(labels) if n else None, ctypes.byref(m)))
        return labels, m.value

    # -- pre-alignment of circular records -----------------------------------------------------------
    def sketch_anchors_device(self, d_bytes, d_offsets, n_records, d_out_sketch, d_out_anchors, d_out_n_kmers=None, params=None, **kw):
        """Enqueues circkit_sketch_anchors_device: sketch_batch_device that also writes d_out_anchors (uint32[n_records << log2_bins],
        device): 2 * start + strand of the k-mer each bin holds, ANCHOR_NONE under an empty bin.  sketch_status() waits."""
        p = params if params is not None else sketch_params(**kw)
        self._check(self._lib.circkit_sketch_anchors_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), ctypes.byref(p),
                                                            _ptr(d_out_sketch), _ptr(d_out_n_kmers), _ptr(d_out_anchors)))

    def prealign_pairs_device(self, d_sketch, d_anchors, d_offsets, n_records, d_pairs, n_pairs, d_windows, d_scores, params=None, **kw):
        """Enqueues circkit_prealign_pairs_device: window p of d_windows (WINDOW_DTYPE, device) rotates and flips record
        d_pairs[2p + 1] onto record d_pairs[2p]; d_scores[2p], d_scores[2p + 1] = (votes, matches).  params: a prealign_params()
        result, or its keywords.  prealign_status() waits."""
        p = params if params is not None else prealign_params(**kw)
        self._check(self._lib.circkit_prealign_pairs_device(self._h, _ptr(d_sketch), _ptr(d_anchors), _ptr(d_offsets), int(n_records), ctypes.byref(p),
                                                            _ptr(d_pairs), int(n_pairs), _ptr(d_windows), _ptr(d_scores)))

    def prealign_status(self):
        """Waits for the last prealign pairs call; returns (aligned pairs, invalid pairs).  Raises CirckitError (INVALID_ARG) when
        a pair named a record that does not exist."""
        a, bad = _u64(0), _u64(0)
        self._check(self._lib.circkit_prealign_status(self._h, ctypes.byref(a), ctypes.byref(bad)))
        return a.value, bad.value

    def prealign_pairs_of_labels_device(self, d_labels, n_records, d_pairs):
        """Enqueues circkit_prealign_pairs_of_labels_device: d_pairs[2i], d_pairs[2i + 1] = (d_labels[i], i) (uint32, device)."""
        self._check(self._lib.circkit_prealign_pairs_of_labels_device(self._h, _ptr(d_labels), int(n_records), _ptr(d_pairs)))

    def prealign_batch(self, data, offsets, pairs, k=21, log2_bins=8, seed=0, min_votes=4):
        """The windows and scores of the pairs (a, b) of a host CSR batch: (windows, scores) with windows an array of WINDOW_DTYPE
        that windows_gather takes as it is and scores an (n_pairs, 2) uint32 array of (votes, matches)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        sp = sketch_params(k=k, log2_bins=log2_bins, seed=seed)
        n, m = len(offsets) - 1, len(pairs)
        windows = np.zeros(m, dtype=WINDOW_DTYPE)
        scores = np.zeros((m, 2), dtype=np.uint32)
        self._check(self._lib.circkit_prealign_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, ctypes.byref(sp),
                                                     _ptr(pairs) if m else None, m, int(min_votes), _ptr(windows) if m else None,
                                                     _ptr(scores) if m else None))
        return windows, scores

    # -- edit distance of record pairs ---------------------------------------------------------------
    def distance_pairs_device(self, d_bytes_a, d_offsets_a, n_a, d_bytes_b, d_offsets_b, n_b, d_pairs, n_pairs, d_out_distance=None,
                              d_out_scores=None, params=None, **kw):
        """Enqueues circkit_distance_pairs_device: d_out_distance[p] (uint32, device, optional) = the edit distance of record
        d_pairs[2p] of batch A and record d_pairs[2p + 1] of batch B when it is at most max_distance, DISTANCE_OVER otherwise;
        d_out_scores[2p], d_out_scores[2p + 1] (optional) = (L - distance, L) with L the longer record's length, what
        cluster_link_device takes.  params: a distance_params() result, or its keywords.  distance_status() waits."""
        p = params if params is not None else distance_params(**kw)
        self._check(self._lib.circkit_distance_pairs_device(self._h, _ptr(d_bytes_a), _ptr(d_offsets_a), int(n_a), _ptr(d_bytes_b), _ptr(d_offsets_b),
                                                            int(n_b), ctypes.byref(p), _ptr(d_pairs), int(n_pairs), _ptr(d_out_distance),
                                                            _ptr(d_out_scores)))

    def distance_status(self):
        """Waits for the last distance pairs call; returns (pairs within max_distance, invalid pairs).  Raises CirckitError
        (INVALID_ARG) when a pair named a record that does not exist or has 2^31 symbols or more."""
        a, bad = _u64(0), _u64(0)
        self._check(self._lib.circkit_distance_status(self._h, ctypes.byref(a), ctypes.byref(bad)))
        return a.value, bad.value

    def distance_pairs(self, data_a, offsets_a, data_b, offsets_b, pairs, max_distance=32):
        """(distance, scores) of the pairs (i, j) of two host CSR batches: a uint32 array with DISTANCE_OVER where the distance
        exceeds max_distance, and an (n_pairs, 2) uint32 array of (L - distance, L).  data_b = offsets_b = None: one batch."""
        data_a = np.ascontiguousarray(data_a, dtype=np.uint8)
        offsets_a = np.ascontiguousarray(offsets_a, dtype=np.uint64)
        same = data_b is None and offsets_b is None
        data_b = data_a if same else np.ascontiguousarray(data_b, dtype=np.uint8)
        offsets_b = offsets_a if same else np.ascontiguousarray(offsets_b, dtype=np.uint64)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        p = distance_params(max_distance=max_distance)
        m = len(pairs)
        dist = np.zeros(m, dtype=np.uint32)
        scores = np.zeros((m, 2), dtype=np.uint32)
        self._check(self._lib.circkit_distance_pairs(self._h, _ptr(data_a) if len(data_a) else None, _ptr(offsets_a), len(offsets_a) - 1,
                                                     _ptr(data_b) if len(data_b) else None, _ptr(offsets_b), len(offsets_b) - 1, ctypes.byref(p),
                                                     _ptr(pairs) if m else None, m, _ptr(dist) if m else None, _ptr(scores) if m else None))
        return dist, scores

    def _records_windows(self, data, offsets, kind, bases=0, percent=0.0):
        """One copy in, the windows of `kind` and their gather on the device, one copy home: (bytes, offsets)."""
        import torch
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n, nb = len(offsets) - 1, int(offsets[-1]) - int(offsets[0])
        dev = torch.device("cuda", self.device)
        cap = {"cat": 2 * nb, "decat": nb // 2}.get(kind, nb)
        with torch.cuda.device(dev):
            # (records without a payload byte still want a pointer: one byte that no window reads)
            d_bytes = torch.from_numpy(data).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
            d_offs = torch.from_numpy(offsets.view(np.int64)).to(dev)
            torch.cuda.current_stream().synchronize()         # the copies are torch's, the kernels the ctx stream's
            d_win = torch.empty(max(n, 1) * WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            self.windows_of_records_device(d_offs, n, kind, d_win, bases=bases, percent=percent)
            self.windows_gather_device(d_bytes, d_offs, n, d_win, n, d_out, cap, d_out_off)
            total, _ = self.windows_status()
            return d_out[:total].cpu().numpy(), d_out_off.cpu().numpy().view(np.uint64)

    def rotate_batch(self, data, offsets, bases=None, percent=None):
        """`circkit rotate --bases` / `--percent` on every record of a host CSR batch (src/rotate.rs:20-43): (bytes, offsets)."""
        if (bases is None) == (percent is None):
            raise ValueError("Must provide either bases or percent")
        if percent is not None:
            return self._records_windows(data, offsets, "rotate_percent", percent=percent)
        if not -2 ** 63 <= int(bases) < 2 ** 63:
            raise ValueError("bases must fit an i64")
        return self._records_windows(data, offsets, "rotate_bases", bases=bases)

    def cat_batch(self, data, offsets):
        """`circkit cat`: every record twice in a row (src/concatenate.rs:10-32)."""
        return self._records_windows(data, offsets, "cat")

    def decat_batch(self, data, offsets):
        """`circkit decat`: the first half of every record (src/concatenate.rs:34-54)."""
        return self._records_windows(data, offsets, "decat")

    def revcomp_batch(self, data, offsets):
        """The reverse complement of every record (bio 1.3.1's dna complement, as canonicalize uses it)."""
        return self._records_windows(data, offsets, "revcomp")

    def orf_sequences(self, data, offsets, include_stop=False, **orf_kw):
        """The ORFs of a host CSR batch of normalized records and their sequences, as `circkit orfs` writes them (`--include-stop`:
        include_stop): (orf_offsets, orfs, seq_bytes, seq_offsets) with orfs an array of ORF_DTYPE and ORF k's sequence
        seq_bytes[seq_offsets[k] .. seq_offsets[k + 1]).  One copy in; the ORF batch, the windows and the gather on the device;
        then the copy home.  Keywords as orf_params."""
        import torch
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        p = orf_params(**orf_kw)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_bytes = torch.from_numpy(data).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
            d_offs = torch.from_numpy(offsets.view(np.int64)).to(dev)
            torch.cuda.current_stream().synchronize()         # the copies are torch's, the kernels the ctx stream's
            d_orf_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            cap = max(n, 1) * 4
            while True:
                d_orfs = torch.empty(cap * ORF_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                self.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, cap, params=p)
                t = _u64(0)
                rc = self._lib.circkit_orfs_status(self._h, ctypes.byref(t))
                if rc == -5 and t.value > cap:                    # grow to the reported total and run again
                    cap = t.value
                    continue
                self._check(rc)
                break
            n_orfs = t.value
            d_win = torch.empty(max(n_orfs, 1) * WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_seq_off = torch.empty(n_orfs + 1, dtype=torch.int64, device=dev)
            self.orfs_windows_device(d_orf_off, d_orfs, n, n_orfs, d_win, include_stop=include_stop)
            # the offsets first (a gather without room reports the total), then the gather into a buffer of that size
            self.windows_gather_device(d_bytes, d_offs, n, d_win, n_orfs, None, 0, d_seq_off)
            total = _u64(0)
            rc = self._lib.circkit_windows_status(self._h, ctypes.byref(total), None)
            if rc != -5:
                self._check(rc)
            d_seq = torch.empty(max(total.value, 1), dtype=torch.uint8, device=dev)
            if total.value:
                self.windows_gather_device(d_bytes, d_offs, n, d_win, n_orfs, d_seq, total.value, d_seq_off)
                self.windows_status()
            orfs = d_orfs.cpu().numpy().view(ORF_DTYPE)[:n_orfs].copy()
            return (d_orf_off.cpu().numpy().view(np.uint64), orfs, d_seq[:total.value].cpu().numpy(), d_seq_off.cpu().numpy().view(np.uint64))

    def orf_proteins(self, data, offsets, include_stop=False, table=1, unknown="X", first_as_m=False, **orf_kw):
        """The ORFs of a host CSR batch of normalized records and their proteins: (orf_offsets, orfs, aa_bytes, aa_offsets), shaped
        like orf_sequences' result, ORF k's protein aa_bytes[aa_offsets[k] .. aa_offsets[k + 1]) the translation of the sequence
        orf_sequences returns for it (with include_stop it ends in the table's stop residue).  One copy in; the ORF batch, the
        windows and the translation on the device; then the copy home.  table / unknown / first_as_m as translate_params, the
        other keywords as orf_params."""
        import torch
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        p = orf_params(**orf_kw)
        tp = translate_params(table=table, unknown=unknown, first_as_m=first_as_m)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            d_bytes = torch.from_numpy(data).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
            d_offs = torch.from_numpy(offsets.view(np.int64)).to(dev)
            torch.cuda.current_stream().synchronize()         # the copies are torch's, the kernels the ctx stream's
            d_orf_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            cap = max(n, 1) * 4
            while True:
                d_orfs = torch.empty(cap * ORF_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                self.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, cap, params=p)
                t = _u64(0)
                rc = self._lib.circkit_orfs_status(self._h, ctypes.byref(t))
                if rc == -5 and t.value > cap:                    # grow to the reported total and run again
                    cap = t.value
                    continue
                self._check(rc)
                break
            n_orfs = t.value
            d_win = torch.empty(max(n_orfs, 1) * WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_aa_off = torch.empty(n_orfs + 1, dtype=torch.int64, device=dev)
            self.orfs_windows_device(d_orf_off, d_orfs, n, n_orfs, d_win, include_stop=include_stop)
            # the offsets first (a translate without room reports the total), then the translate into a buffer of that size
            self.windows_translate_device(d_bytes, d_offs, n, d_win, n_orfs, None, 0, d_aa_off, params=tp)
            total = _u64(0)
            rc = self._lib.circkit_translate_status(self._h, ctypes.byref(total), None)
            if rc != -5:
                self._check(rc)
            d_aa = torch.empty(max(total.value, 1), dtype=torch.uint8, device=dev)
            if total.value:
                self.windows_translate_device(d_bytes, d_offs, n, d_win, n_orfs, d_aa, total.value, d_aa_off, params=tp)
                self.translate_status()
            orfs = d_orfs.cpu().numpy().view(ORF_DTYPE)[:n_orfs].copy()
            return (d_orf_off.cpu().numpy().view(np.uint64), orfs, d_aa[:total.value].cpu().numpy(), d_aa_off.cpu().numpy().view(np.uint64))

    # -- monomerize -----------------------------------------------------------------------------
    def monomerize_batch_device(self, d_bytes, d_offsets, n_records, d_end, params=None, **kw):
        """Enqueues circkit_monomerize_batch_device: d_end (uint32[n_records], device) gets every record's end index or
        MONOMER_NONE once the ctx stream has run past it."""
        p = params if params is not None else monomerize_params(**kw)
        self._check(self._lib.circkit_monomerize_batch_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records),
                                                              ctypes.byref(p), _ptr(d_end)))

    def monomerize_batch(self, data, offsets, seed_len=10, max_mismatch=None, min_identity=None, sensitive=False):
        """End index of the first monomer of every record of a host CSR batch: a uint32 array, MONOMER_NONE where the
        reference returns None (last_monomer_end_index, or its sensitive form)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        p = monomerize_params(seed_len, max_mismatch, min_identity, sensitive)
        out = np.full(max(n, 1), MONOMER_NONE, dtype=np.uint32)
        self._check(self._lib.circkit_monomerize_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n,
                                                       ctypes.byref(p), _ptr(out)))
        return out[:n]

    def monomers_compact_device(self, d_bytes, d_offsets, n_records, d_end, d_out_bytes, d_out_offsets, d_out_src, d_full_len=None,
                                d_kept_end=None, filter=None, **kw):
        """Enqueues circkit_monomers_compact_device: the writer's filters (monomer_filter keywords, or filter=) on the end
        indices d_end, and the written monomers packed into the CSR batch d_out_bytes / d_out_offsets, with d_out_src[j] =
        the input index of output record j.  monomers_status() waits and returns the totals."""
        f = filter if filter is not None else monomer_filter(**kw)
        self._check(self._lib.circkit_monomers_compact_device(self._h, _ptr(d_bytes), _ptr(d_offsets), int(n_records), _ptr(d_end),
                                                              _ptr(d_full_len), ctypes.byref(f),
                                                              _ptr(d_out_bytes), _ptr(d_out_offsets), _ptr(d_out_src), _ptr(d_kept_end)))

    def monomers_status(self):
        """Waits for the last compact; returns (number of written records, their bytes)."""
        m, b = _u64(0), _u64(0)
        self._check(self._lib.circkit_monomers_status(self._h, ctypes.byref(m), ctypes.byref(b)))
        return m.value, b.value

    def monomers_batch(self, data, offsets, full_len=None, seed_len=10, max_mismatch=None, min_identity=None, sensitive=False, **filter):
        """The monomers `circkit monomerize` writes for a host CSR batch of normalized records, as a CSR batch: (out_data,
        out_offsets, out_src, kept_end).  out_src[j] = the input index of output record j; kept_end[i] = the end index of input
        record i that survived the filters (monomer_filter keywords), MONOMER_NONE otherwise.  full_len: full_seq().len() per
        record where it differs from the normalized length."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        p = monomerize_params(seed_len, max_mismatch, min_identity, sensitive)
        f = monomer_filter(**filter)
        fl = np.ascontiguousarray(full_len, dtype=np.uint64) if full_len is not None else None
        if fl is not None and len(fl) != n:
            raise ValueError("full_len must have one entry per record")
        out = np.empty(max(len(data), 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        out_src = np.zeros(max(n, 1), dtype=np.uint64)
        kept = np.full(max(n, 1), MONOMER_NONE, dtype=np.uint32)
        m = _u64(0)
        self._check(self._lib.circkit_monomers_batch(self._h, _ptr(data) if len(data) else None, _ptr(offsets), n, ctypes.byref(p),
                                                     ctypes.byref(f), _ptr(fl), _ptr(out), _ptr(out_off), _ptr(out_src), _ptr(kept),
                                                     ctypes.byref(m)))
        m = m.value
        return out[:int(out_off[m])], out_off[:m + 1], out_src[:m], kept[:n]

    def monomer_end_index(self, s, seed_len=10, max_mismatch=None, min_identity=None, sensitive=False):
        """lib/src/monomerize.rs:97 / :122 on any bytes: the end index, or None."""
        s = bytes(s)
        buf = ctypes.create_string_buffer(s, max(len(s), 1))
        p = monomerize_params(seed_len, max_mismatch, min_identity, sensitive)
        end, found = _sz(0), _i(0)
        self._check(self._lib.circkit_monomer_end_index(self._h, ctypes.addressof(buf), len(s), ctypes.byref(p),
                                                        ctypes.byref(end), ctypes.byref(found)))
        return end.value if found.value else None

    def monomerize(self, s, **kw):
        """Monomerizer::monomerize / monomerize_sensitive (lib/src/monomerize.rs:138, :146): the monomer's bytes."""
        s = bytes(s)
        e = self.monomer_end_index(s, **kw)
        return s if e is None else s[:e]

    # -- single record: the lib-crate API --------------------------------------------------------
    def _single(self, fn, s):
        s = bytes(s)
        buf = ctypes.create_string_buffer(s, max(len(s), 1))
        out = ctypes.create_string_buffer(max(len(s), 1))
        self._check(fn(self._h, ctypes.addressof(buf), len(s), ctypes.addressof(out)))
        return out.raw[:len(s)]

    def lmsr_index(self, s):
        s = bytes(s)
        buf = ctypes.create_string_buffer(s, max(len(s), 1))
        r = _sz(0)
        self._check(self._lib.circkit_lmsr_index(self._h, ctypes.addressof(buf), len(s), ctypes.byref(r)))
        return r.value

    def lmsr(self, s):
        return self._single(self._lib.circkit_lmsr, s)

    def canonicalize(self, s):
        return self._single(self._lib.circkit_canonicalize, s)

    def xxh3_64(self, s):
        s = bytes(s)
        buf = ctypes.create_string_buffer(s, max(len(s), 1))
        r = _u64(0)
        self._check(self._lib.circkit_xxh3_64(self._h, ctypes.addressof(buf), len(s), ctypes.byref(r)))
        return r.value


def normalize(s):
    """needletail::sequence::normalize(seq, false): returns (bytes, changed)."""
    lib = load_library()
    s = bytes(s)
    buf = ctypes.create_string_buffer(s, max(len(s), 1))
    out = ctypes.create_string_buffer(max(len(s), 1))
    ch = _i(0)
    m = lib.circkit_normalize(ctypes.addressof(buf), len(s), ctypes.addressof(out), ctypes.byref(ch))
    return out.raw[:m], bool(ch.value)


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def lmsr_index(s):
    return default_context().lmsr_index(s)


def lmsr(s):
    return default_context().lmsr(s)


def canonicalize(s):
    return default_context().canonicalize(s)


def xxh3_64(s):
    return default_context().xxh3_64(s)


def find_orfs(s):
    return default_context().find_orfs(s)


def monomer_end_index(s, **kw):
    return default_context().monomer_end_index(s, **kw)


def monomerize(s, **kw):
    return default_context().monomerize(s, **kw)


def monomers_batch(data, offsets, **kw):
    return default_context().monomers_batch(data, offsets, **kw)


def uniq_batch(data, offsets, **kw):
    return default_context().uniq_batch(data, offsets, **kw)


def rotate_batch(data, offsets, bases=None, percent=None):
    return default_context().rotate_batch(data, offsets, bases=bases, percent=percent)


def cat_batch(data, offsets):
    return default_context().cat_batch(data, offsets)


def decat_batch(data, offsets):
    return default_context().decat_batch(data, offsets)


def revcomp_batch(data, offsets):
    return default_context().revcomp_batch(data, offsets)


def orf_sequences(data, offsets, include_stop=False, **orf_params):
    return default_context().orf_sequences(data, offsets, include_stop=include_stop, **orf_params)


def windows_translate(data, offsets, windows, **kw):
    return default_context().windows_translate(data, offsets, windows, **kw)


def sketch_batch(seqs, k=21, log2_bins=8, seed=0):
    """The cyclic k-mer MinHash sketches of a list of normalized records (bytes): an (n, 1 << log2_bins) uint64 array, rotation-
    and strand-invariant row by row, and the records' valid k-mer counts."""
    seqs = [bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    return default_context().sketch_batch(data, offsets, k=k, log2_bins=log2_bins, seed=seed)


def sketch_similarity(sk_a, sk_b, pairs):
    """(match, filled) of every pair (i, j) of rows of two sketch arrays: match / filled estimates the Jaccard index of the two
    records' canonical cyclic k-mer sets."""
    return default_context().sketch_compare(sk_a, sk_b, pairs)


def cluster_batch(seqs, k=21, log2_bins=8, seed=0, **cluster):
    """Single-linkage clusters of a list of normalized records (bytes) over their sketches: (labels, n_clusters), labels[i] =
    the smallest index in record i's cluster.  The keywords of cluster_params choose the bands and the threshold."""
    seqs = [bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    return default_context().cluster_batch(data, offsets, k=k, log2_bins=log2_bins, seed=seed, **cluster)


def _csr_of(seqs):
    seqs = [bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets


def sketch_anchors(seqs, k=21, log2_bins=8, seed=0):
    """sketch_batch with the anchors: (rows, counts, anchors), anchors an (n, 1 << log2_bins) uint32 array holding 2 * start +
    strand of the k-mer every bin keeps (the smallest start), ANCHOR_NONE under an empty bin."""
    import torch
    data, offsets = _csr_of(seqs)
    ctx = default_context()
    n, bins = len(offsets) - 1, 1 << int(log2_bins)
    dev = torch.device("cuda", ctx.device)
    with torch.cuda.device(dev):
        d_data = torch.from_numpy(data.copy()).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
        d_offs = torch.from_numpy(offsets.view(np.int64)).to(dev)
        d_rows = torch.empty(max(n * bins, 1), dtype=torch.int64, device=dev)
        d_anchors = torch.empty(max(n * bins, 1), dtype=torch.int32, device=dev)
        d_counts = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        torch.cuda.current_stream().synchronize()             # the copies are torch's, the kernels the ctx stream's
        ctx.sketch_anchors_device(d_data, d_offs, n, d_rows, d_anchors, d_counts, k=k, log2_bins=log2_bins, seed=seed)
        ctx.sketch_status()
        rows = d_rows[:n * bins].cpu().numpy().view(np.uint64).reshape(n, bins)
        counts = d_counts[:n].cpu().numpy().view(np.uint32)
        anchors = d_anchors[:n * bins].cpu().numpy().view(np.uint32).reshape(n, bins)
    return rows, counts, anchors


def prealign_batch(seqs, pairs, k=21, log2_bins=8, seed=0, min_votes=4):
    """For every pair (a, b) of a list of normalized records (bytes), the window that rotates and flips b onto a, and
    (votes, matches): (windows, scores).  The windows are a WINDOW_DTYPE array that windows_gather takes as it is; a pair with
    fewer than min_votes agreeing bins gets the identity window."""
    data, offsets = _csr_of(seqs)
    return default_context().prealign_batch(data, offsets, pairs, k=k, log2_bins=log2_bins, seed=seed, min_votes=min_votes)


def edit_distances(seqs_a, seqs_b, pairs, max_distance=32):
    """The edit distance of record i of seqs_a and record j of seqs_b (seqs_b = None: of seqs_a too) for every pair (i, j): a
    uint32 array, DISTANCE_OVER where the distance exceeds max_distance (0 .. 255).  Symbols are bytes as they are."""
    data_a, offsets_a = _csr_of(seqs_a)
    data_b, offsets_b = (None, None) if seqs_b is None else _csr_of(seqs_b)
    return default_context().distance_pairs(data_a, offsets_a, data_b, offsets_b, pairs, max_distance=max_distance)[0]


def orf_proteins(data, offsets, include_stop=False, **kw):
    return default_context().orf_proteins(data, offsets, include_stop=include_stop, **kw)


def fasta_parse_gpu(text, first_chunk=True, final_chunk=True, keep_on_device=False):
    """fasta_parse with the parse on the GPU (Context.fasta_parse_text): the same four results."""
    return default_context().fasta_parse_text(text, first_chunk=first_chunk, final_chunk=final_chunk, keep_on_device=keep_on_device)


def fasta_write_gpu(text, head, **kw):
    """FASTA text written on the GPU (Context.fasta_write_text): (bytes, out_offsets)."""
    return default_context().fasta_write_text(text, head, **kw)


def fasta_parse(text, first_chunk=True, final_chunk=True):
    """FASTA text -> (records, normalized_bytes, offsets, consumed); records = [(head, raw_seq)] with seq_io
    semantics.  Host logic (circkit_fasta_parse); raises ValueError on a format error."""
    lib = load_library()
    text = bytes(text)
    buf = ctypes.create_string_buffer(text, max(len(text), 1))
    h = _vp()
    consumed = _sz(0)
    rc = lib.circkit_fasta_parse(ctypes.addressof(buf), len(text), int(first_chunk), int(final_chunk), ctypes.byref(h),
                                 ctypes.byref(consumed))
    try:
        if rc != OK:
            raise ValueError(lib.circkit_fasta_error(h).decode() if h else "fasta parse failed")
        n = lib.circkit_fasta_n_records(h)
        offs = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_offsets(h), ctypes.POINTER(ctypes.c_uint64)),
                                     shape=(n + 1,)).copy()
        total = int(offs[-1])
        data = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_bytes(h), ctypes.POINTER(ctypes.c_uint8)),
                                     shape=(max(total, 1),)).copy()[:total]
        recs = []
        ho, hl, ro, rl = _sz(0), _sz(0), _sz(0), _sz(0)
        for i in range(n):
            lib.circkit_fasta_record(h, i, ctypes.byref(ho), ctypes.byref(hl), ctypes.byref(ro), ctypes.byref(rl))
            recs.append((text[ho.value:ho.value + hl.value], text[ro.value:ro.value + rl.value]))
        return recs, data, offs, consumed.value
    finally:
        if h:
            lib.circkit_fasta_free(h)
