"""circkit_amd -- MI355X (gfx950) drop-in for circkit's canonicalize / uniq hot path.

csrc/      hand-written HIP kernels + the C ABI (include/circkit.h) + the C++ FASTA host
api.py     ctypes mirror of the reference's lib-crate API over that C ABI
monomerize.py  `circkit monomerize` over the GPU batch call (also `python -m circkit_amd.monomerize`); the module is
           callable: circkit_amd.monomerize(s, ...) is Monomerizer::monomerize on one record
cluster.py  text -> sketch -> candidates -> compare -> link -> representatives as FASTA, on the device (also
           `python -m circkit_amd.cluster`)
prealign.py  the same chain, then every record rotated and flipped onto its cluster's representative (also
           `python -m circkit_amd.prealign`)
"""
from .api import (ANCHOR_NONE, DISTANCE_MAX, DISTANCE_OVER, GENETIC_CODES, SKETCH_EMPTY, CirckitError, Context, canonicalize, cat_batch, cluster_batch, cluster_params, decat_batch, default_context, distance_params, edit_distances, fasta_parse_gpu, fasta_write_gpu, find_orfs,  # noqa: F401
                  lmsr,
                  lmsr_index, load_library, monomer_end_index, monomer_filter, monomerize_params, monomers_batch, normalize, orf_params,
                  orf_proteins, orf_sequences, prealign_batch, prealign_params, revcomp_batch, rotate_batch, sketch_anchors, sketch_batch, sketch_params, sketch_similarity, translate_params, uniq_batch, windows_translate, xxh3_64)
from . import uniq  # noqa: F401,E402


def __getattr__(name):
    # loaded on first use, so that `python -m circkit_amd.monomerize` does not find its module imported already
    if name in ("monomerize", "cluster", "prealign"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
