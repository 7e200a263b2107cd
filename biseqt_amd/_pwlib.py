"""ctypes binding of biseqt_amd/pwlib/pwlib.so (the HIP library; C ABI in include/pwlib.h,
include/pw_batch.h, include/pw_txsum.h, include/pw_cigar.h, include/pw_pileup.h, include/pw_polish.h, include/pw_graph.h, include/pw_consensus.h and the seed headers include/pw_seeds.h, pw_mseeds.h, pw_qseeds.h, pw_overlap.h).

The reference binds its C library with cffi in ABI mode (``biseqt/pw.py:45-69``); cffi is not
available in this image, so the same structs are declared with ctypes -- field for field the layout of
``pwlib.h`` (checked by ``check_layout``).  There is no fallback: if the shared object is missing the
import fails with instructions, and every computing call goes to the GPU kernels.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PWLIB_SO = os.environ.get('PWLIB_SO', os.path.join(HERE, 'pwlib', 'pwlib.so'))   # override: A/B experiments only
PWLIB_H = os.path.join(HERE, 'pwlib', 'pwlib.h')

# enum values of include/pwlib.h (reference pwlib.h:30-33, 39-54, 60-65)
STD_MODE, BANDED_MODE = 0, 1
GLOBAL, LOCAL, START_ANCHORED, END_ANCHORED, OVERLAP, START_ANCHORED_OVERLAP, \
    END_ANCHORED_OVERLAP = range(7)
B_GLOBAL, B_LOCAL, B_OVERLAP = range(3)


class intpair(C.Structure):
    _fields_ = [('i', C.c_int), ('j', C.c_int)]


class alnscores(C.Structure):
    _fields_ = [('subst_scores', C.POINTER(C.POINTER(C.c_double))),
                ('gap_open_score', C.c_double),
                ('gap_extend_score', C.c_double)]


class alnframe(C.Structure):
    _fields_ = [('origin', C.POINTER(C.c_int)),
                ('mutant', C.POINTER(C.c_int)),
                ('origin_range', intpair),
                ('mutant_range', intpair)]


class std_alnparams(C.Structure):
    _fields_ = [('type', C.c_int)]


class banded_alnparams(C.Structure):
    _fields_ = [('type', C.c_int), ('dmin', C.c_int), ('dmax', C.c_int)]


class alnprob(C.Structure):
    _fields_ = [('frame', C.POINTER(alnframe)),
                ('scores', C.POINTER(alnscores)),
                ('max_new_mins', C.c_int),
                ('mode', C.c_int),
                ('params', C.c_void_p)]      # union { std_alnparams*, banded_alnparams* }


class alnchoice(C.Structure):
    pass


alnchoice._fields_ = [('op', C.c_char),
                      ('score', C.c_double),
                      ('base', C.POINTER(alnchoice)),
                      ('mins_cd', C.c_int),
                      ('cur_min', C.c_int)]


class dpcell(C.Structure):
    _fields_ = [('num_choices', C.c_int),
                ('choices', C.POINTER(alnchoice))]


class dptable(C.Structure):
    _fields_ = [('cells', C.POINTER(C.POINTER(dpcell))),
                ('num_rows', C.c_int),
                ('row_lens', C.POINTER(C.c_int)),
                ('prob', C.POINTER(alnprob))]


class alignment(C.Structure):
    _fields_ = [('origin_idx', C.c_int),
                ('mutant_idx', C.c_int),
                ('score', C.c_double),
                ('transcript', C.c_char_p)]


# ---- batch API (include/pw_batch.h) ----
class pw_scoring(C.Structure):
    _fields_ = [('mode', C.c_int), ('type', C.c_int), ('alphabet_len', C.c_int),
                ('subst', C.POINTER(C.c_double)), ('go', C.c_double), ('ge', C.c_double)]


class pw_pair(C.Structure):
    _fields_ = [('origin_off', C.c_uint64), ('mutant_off', C.c_uint64),
                ('origin_len', C.c_int32), ('mutant_len', C.c_int32),
                ('dmin', C.c_int32), ('dmax', C.c_int32)]


class pw_result(C.Structure):
    _fields_ = [('score', C.c_double), ('opt_i', C.c_int32), ('opt_j', C.c_int32),
                ('origin_idx', C.c_int32), ('mutant_idx', C.c_int32),
                ('tx_len', C.c_int32), ('status', C.c_int32)]


# ---- alignment summaries (include/pw_txsum.h) ----
class pw_tx_summary(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ('n_match', 'n_subst', 'n_ins', 'n_del', 'n_gaps', 'first_match', 'last_match',
                                         'head_origin', 'head_mutant', 'tail_origin', 'tail_mutant', 'flags')]


# ---- pileups (include/pw_pileup.h) ----
class pw_pileup_site(C.Structure):
    _fields_ = [('depth', C.c_uint32), ('call', C.c_uint8), ('ref', C.c_uint8), ('flags', C.c_uint16)]


# ---- read correction (include/pw_polish.h) ----
class pw_polish_stats(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ('kept', 'substituted', 'deleted', 'inserted')]


# ---- the overlap graph (include/pw_graph.h) ----
class pw_graph_overlap(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ('a', 'b', 'strand', 'cls', 'a_beg', 'a_end', 'b_beg', 'b_end', 'n_match', 'n_ops')]


class pw_graph_params(C.Structure):
    _fields_ = [('max_hang', C.c_int32), ('min_overlap', C.c_int32), ('fuzz', C.c_int32), ('pad_', C.c_int32),
                ('int_frac', C.c_double), ('min_identity', C.c_double)]


class pw_graph_clean_params(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ('max_tip_reads', 'max_bubble_reads', 'rounds', 'pad_')]


class pw_graph_arc(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ('v', 'w', 'len', 'ol', 'src', 'flags')]


class pw_unitig(C.Structure):
    _fields_ = [('first_member', C.c_int64), ('length', C.c_int64), ('n_members', C.c_int32), ('head', C.c_int32),
                ('circular', C.c_int32), ('pad_', C.c_int32)]


class pw_unitig_member(C.Structure):
    _fields_ = [('vertex', C.c_int32), ('advance', C.c_int32), ('offset', C.c_int64)]


# ---- the consensus layout (include/pw_consensus.h) ----
class pw_cons_place(C.Structure):
    _fields_ = [('unitig', C.c_int32), ('rev', C.c_int32), ('pos', C.c_int64), ('root', C.c_int32), ('depth', C.c_int32)]


class pw_cons_task(C.Structure):
    _fields_ = [('col0', C.c_int64), ('mut_off', C.c_int64)] + [(f, C.c_int32) for f in ('read', 'win_len', 'dmin', 'dmax', 'rev', 'pad_')]


PW_TXSUM_DONE = 1
PW_ST_TRACED, PW_ST_EMPTY, PW_ST_PANICK, PW_ST_BADPATH = 1, 2, 4, 8
PW_FLAG_DUMP_SCORES, PW_FLAG_FORCE_F64, PW_FLAG_FORCE_GENERIC, PW_FLAG_PROFILE = 1, 2, 4, 8
PW_FLAG_NO_PACKED16 = 16
PW_FLAG_FORCE_TILED = 32
PW_FLAG_FORCE_STRIP = 64
PW_FLAG_SHARED_ARENA = 128
PW_FLAG_NO_STRIP = 256

SIZEOF = dict(intpair=8, alnscores=24, alnframe=32, std_alnparams=4, banded_alnparams=12,
              alnprob=32, alnchoice=32, dpcell=16, dptable=32, alignment=24,
              pw_scoring=40, pw_pair=32, pw_result=32, pw_tx_summary=48, pw_pileup_site=8, pw_polish_stats=16,
              pw_graph_overlap=40, pw_graph_params=32, pw_graph_clean_params=16, pw_graph_arc=24, pw_unitig=32, pw_unitig_member=16, pw_cons_place=24, pw_cons_task=40)

# every symbol include/pwlib.h and include/pw_batch.h declare
EXPORTS = ['dptable_init', 'dptable_solve', 'dptable_traceback', 'dptable_free',
           'pw_last_error', 'pw_device_count', 'pw_device_memory', 'pw_pool_trim', 'pw_batch_create', 'pw_batch_destroy',
           'pw_batch_init_rc', 'pw_batch_band', 'pw_batch_pair_cells', 'pw_batch_cells',
           'pw_batch_algorithmic_bytes', 'pw_batch_score_type', 'pw_batch_kernel_name', 'pw_batch_upload_arena',
           'pw_batch_arena_device', 'pw_arena_upload', 'pw_arena_free', 'pw_batch_share_arena', 'pw_host_alloc', 'pw_host_free', 'pw_batch_upload_arena_async',
           'pw_batch_results_async', 'pw_batch_transcripts_async', 'pw_batch_solve', 'pw_batch_traceback',
           'pw_batch_traceback_from', 'pw_batch_sync', 'pw_batch_results_device',
           'pw_batch_transcripts_device', 'pw_batch_transcripts_bytes', 'pw_batch_tx_slot',
           'pw_batch_results', 'pw_batch_transcripts', 'pw_batch_scores', 'pw_batch_masks', 'pw_batch_table', 'pw_batch_fill_ms',
           'pw_batch_trace_ms', 'pw_batch_pack_transcripts', 'pw_batch_packed_device', 'pw_batch_packed_offsets_device',
           'pw_batch_packed_total_async', 'pw_batch_packed', 'pw_plan_only']
# every symbol include/pw_txsum.h declares
TXSUM_EXPORTS = ['pw_batch_summarize', 'pw_batch_summaries_device', 'pw_batch_summaries_async', 'pw_batch_summaries',
                 'pw_tx_summarize_packed']
# every symbol and constant include/pw_cigar.h declares
CIGAR_EXPORTS = ['pw_batch_cigars', 'pw_batch_cigar_runs_device', 'pw_batch_cigar_offsets_device', 'pw_batch_cigar_total', 'pw_batch_cigar',
                 'pw_tx_cigar_packed']
PW_CIGAR_EXTENDED, PW_CIGAR_CLASSIC = 0, 1
PW_CIGAR_OP_M, PW_CIGAR_OP_I, PW_CIGAR_OP_D, PW_CIGAR_OP_EQ, PW_CIGAR_OP_X = 0, 1, 2, 7, 8
PW_CIGAR_MAX_LEN = 1 << 28
# every symbol and constant include/pw_pileup.h declares
PILEUP_EXPORTS = ['pw_pileup_create', 'pw_pileup_destroy', 'pw_pileup_clear', 'pw_batch_pileup_add', 'pw_pileup_counts_device',
                  'pw_pileup_counts', 'pw_pileup_set_counts', 'pw_pileup_call', 'pw_pileup_sites_device', 'pw_pileup_sites']
PW_PILEUP_COVERED, PW_PILEUP_DIFFERS, PW_PILEUP_INSERT = 1, 2, 4
# every symbol and constant include/pw_polish.h declares
POLISH_EXPORTS = ['pw_pileup_create_ins', 'pw_pileup_ins_slots', 'pw_pileup_ins_counts_device', 'pw_pileup_ins_counts',
                  'pw_batch_pileup_add_sides', 'pw_pileup_add_letters', 'pw_pileup_polish', 'pw_pileup_polished_total',
                  'pw_pileup_polished_offsets', 'pw_pileup_polished_letters', 'pw_pileup_polished_stats',
                  'pw_pileup_polished_letters_device', 'pw_pileup_polished_offsets_device']
PW_POLISH_MAX_SLOTS = 8
PW_SIDE_ORIGIN, PW_SIDE_MUTANT, PW_SIDE_BOTH = 1, 2, 3
# every symbol and constant include/pw_graph.h declares
GRAPH_EXPORTS = ['pw_graph_create', 'pw_graph_free', 'pw_graph_num_overlaps', 'pw_graph_device_bytes', 'pw_graph_add_overlaps', 'pw_batch_graph_add', 'pw_graph_build', 'pw_graph_build_clean', 'pw_graph_dropped', 'pw_graph_dropped_device', 'pw_graph_num_arcs', 'pw_graph_num_unitigs',
                 'pw_graph_num_members', 'pw_graph_reduce_ms', 'pw_graph_overlaps', 'pw_graph_contained', 'pw_graph_arcs', 'pw_graph_rows', 'pw_graph_unitigs',
                 'pw_graph_members', 'pw_graph_overlaps_device', 'pw_graph_contained_device', 'pw_graph_arcs_device',
                 'pw_graph_rows_device', 'pw_graph_unitigs_device', 'pw_graph_members_device', 'pw_graph_contigs',
                 'pw_graph_contig_total', 'pw_graph_contig_offsets', 'pw_graph_contig_letters', 'pw_graph_contig_letters_device',
                 'pw_graph_contig_offsets_device']
# every symbol include/pw_consensus.h declares
CONSENSUS_EXPORTS = ['pw_graph_place', 'pw_graph_placements', 'pw_graph_placements_device', 'pw_graph_consensus_layout',
                     'pw_graph_cons_num_tasks', 'pw_graph_cons_num_cols', 'pw_graph_cons_arena_bytes', 'pw_graph_cons_cstart',
                     'pw_graph_cons_tasks', 'pw_graph_cons_cstart_device', 'pw_graph_cons_tasks_device', 'pw_graph_cons_arena_device']
# include/pw_rounds.h
ROUNDS_EXPORTS = ['pw_pileup_polish_columns', 'pw_pileup_colmap_device', 'pw_pileup_colmap', 'pw_graph_consensus_relayout',
                  'pw_graph_cons_round', 'pw_graph_cons_positions', 'pw_graph_cons_lengths']
PW_OVL_NONE, PW_OVL_WEAK, PW_OVL_INTERNAL, PW_OVL_A_CONTAINED, PW_OVL_B_CONTAINED, PW_OVL_A_TO_B, PW_OVL_B_TO_A = range(7)
PW_ARC_REDUCED, PW_ARC_REMOVED, PW_ARC_CHAIN, PW_ARC_DROPPED = 1, 2, 4, 8
# every symbol include/pw_seeds.h declares
SEED_EXPORTS = ['pw_seeds_create', 'pw_seeds_build', 'pw_seeds_num_rows', 'pw_seeds_is_self', 'pw_seeds_rows_device',
                'pw_seeds_rows', 'pw_seeds_count', 'pw_seeds_kmers', 'pw_seeds_band_neighbours', 'pw_seeds_graph_build', 'pw_seeds_graph_num_points', 'pw_seeds_graph_points',
                'pw_seeds_graph_counts', 'pw_seeds_graph_fetch', 'pw_seeds_graph_components', 'pw_seeds_build_ms',
                'pw_seeds_algorithmic_bytes', 'pw_seeds_destroy', 'pw_seeds_last_error']

# every symbol include/pw_mseeds.h declares
MSEED_EXPORTS = ['pw_mseeds_create', 'pw_mseeds_build', 'pw_mseeds_num_seqs', 'pw_mseeds_num_rows', 'pw_mseeds_rows_device',
                 'pw_mseeds_rows', 'pw_mseeds_count_many', 'pw_mseeds_graph_build', 'pw_mseeds_graph_counts',
                 'pw_mseeds_graph_fetch', 'pw_mseeds_graph_components', 'pw_mseeds_build_ms', 'pw_mseeds_graph_ms',
                 'pw_mseeds_components_ms', 'pw_mseeds_count_ms', 'pw_mseeds_algorithmic_bytes', 'pw_mseeds_destroy',
                 'pw_mseeds_last_error']

# every symbol include/pw_qseeds.h declares
QSEED_EXPORTS = ['pw_qseeds_create', 'pw_qseeds_build', 'pw_qseeds_build_stranded', 'pw_qseeds_num_queries', 'pw_qseeds_num_rows', 'pw_qseeds_rows_device',
                 'pw_qseeds_rows', 'pw_qseeds_row_offsets', 'pw_qseeds_count_boxes', 'pw_qseeds_graph_build',
                 'pw_qseeds_graph_counts', 'pw_qseeds_graph_fetch', 'pw_qseeds_graph_components', 'pw_qseeds_build_ms',
                 'pw_qseeds_graph_ms', 'pw_qseeds_components_ms', 'pw_qseeds_count_ms', 'pw_qseeds_components_rounds',
                 'pw_qseeds_destroy', 'pw_qseeds_last_error']

# every symbol include/pw_overlap.h declares
OVERLAP_EXPORTS = ['pw_overlap_bands', 'pw_overlap_all_pairs', 'pw_overlap_last_ms', 'pw_overlap_last_error',
                   'pw_overlap_bands_stranded', 'pw_overlap_all_pairs_stranded', 'pw_overlap_all_pairs_capped', 'pw_overlap_arena_upload',
                   'pw_overlap_arena_read', 'pw_overlap_all_pairs_sampled']
PW_STRAND_PLUS, PW_STRAND_MINUS, PW_STRAND_BOTH = 1, 2, 3
# every symbol include/pw_kmers.h declares
KMERS_EXPORTS = ['pw_kmers_create', 'pw_kmers_build', 'pw_kmers_num_entries', 'pw_kmers_num_distinct', 'pw_kmers_distinct',
                 'pw_kmers_lookup', 'pw_kmers_hits', 'pw_kmers_spectrum', 'pw_kmers_occurrences', 'pw_kmers_destroy',
                 'pw_kmers_last_ms', 'pw_kmers_last_error', 'pw_kmers_build_sampled', 'pw_kmers_num_positions', 'pw_kmers_rows',
                 'pw_kmers_read_starts']


class pw_overlap_cap_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ('entries', 'masked_entries', 'distinct_masked', 'seeds_kept', 'seeds_dropped')]


class pw_overlap_sample_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ('positions', 'sampled')]


class pw_read_pair(C.Structure):
    _fields_ = [('s_off', C.c_uint64), ('t_off', C.c_uint64), ('s_len', C.c_int32), ('t_len', C.c_int32)]


def check_layout():
    for name, size in SIZEOF.items():
        assert C.sizeof(globals()[name]) == size, (name, C.sizeof(globals()[name]), size)


_lib = None


def _bind_hip_runtime():
    """One HIP runtime per process.  ``pwlib.so`` needs ``libamdhip64.so.7``; a PyTorch wheel bundles its own copy of
    that library (same SONAME) and two HIP / HSA runtimes in one process cannot both find the GPU.  If ``pwlib.so`` is
    loaded first it would pull in the system runtime and a later ``import torch`` would bring the second one, so when a
    torch installation with a bundled runtime exists and none is mapped yet, that copy is loaded first (RTLD_GLOBAL):
    ``pwlib.so`` then binds to it by SONAME, and torch, imported later or never, finds its own library already there.
    ``PWLIB_HIP_RUNTIME=system`` keeps the system runtime, ``PWLIB_HIP_RUNTIME=/path/libamdhip64.so`` picks one."""
    import sys
    choice = os.environ.get('PWLIB_HIP_RUNTIME', '')
    if choice == 'system':
        return None
    try:
        with open('/proc/self/maps') as f:
            if 'libamdhip64' in f.read():
                return None                      # a runtime is mapped already (torch imported first): bind to it
    except OSError:
        pass
    path = choice
    if not path:
        if 'torch' in sys.modules:
            return None
        try:
            import importlib.util
            spec = importlib.util.find_spec('torch')             # locates the package without importing it
        except (ImportError, ValueError):
            spec = None
        if spec is None or not spec.origin:
            return None
        path = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if not os.path.exists(path):
        return None
    try:
        return C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        return None


def load():
    """dlopen pwlib.so and declare its prototypes.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(PWLIB_SO):
        raise ImportError('%s is missing: build it with `python -m biseqt_amd.csrc.build` '
                          '(hipcc, gfx950); there is no CPU fallback' % PWLIB_SO)
    _bind_hip_runtime()
    lib = C.CDLL(PWLIB_SO)
    P = C.POINTER
    lib.dptable_init.argtypes = [P(dptable)]
    lib.dptable_init.restype = C.c_int
    lib.dptable_solve.argtypes = [P(dptable)]
    lib.dptable_solve.restype = intpair
    lib.dptable_traceback.argtypes = [P(dptable), intpair]
    lib.dptable_traceback.restype = P(alignment)
    lib.dptable_free.argtypes = [P(dptable)]
    lib.dptable_free.restype = None
    lib.pw_last_error.restype = C.c_char_p
    lib.pw_device_count.restype = C.c_int
    lib.pw_device_memory.argtypes = [C.c_int, P(C.c_uint64), P(C.c_uint64)]
    lib.pw_pool_trim.restype = None
    lib.pw_batch_create.argtypes = [C.c_int, P(pw_scoring), C.c_int32, P(pw_pair), C.c_uint64, C.c_uint32]
    lib.pw_batch_create.restype = C.c_void_p
    lib.pw_batch_destroy.argtypes = [C.c_void_p]
    lib.pw_batch_destroy.restype = None
    lib.pw_batch_init_rc.argtypes = [C.c_void_p, C.c_int32]
    lib.pw_batch_band.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    lib.pw_batch_pair_cells.argtypes = [C.c_void_p, C.c_int32]
    lib.pw_batch_pair_cells.restype = C.c_int64
    lib.pw_batch_cells.argtypes = [C.c_void_p]
    lib.pw_batch_cells.restype = C.c_int64
    lib.pw_batch_algorithmic_bytes.argtypes = [C.c_void_p]
    lib.pw_batch_algorithmic_bytes.restype = C.c_int64
    lib.pw_batch_score_type.argtypes = [C.c_void_p]
    lib.pw_batch_kernel_name.argtypes = [C.c_void_p]
    lib.pw_batch_kernel_name.restype = C.c_char_p
    lib.pw_batch_upload_arena.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    lib.pw_batch_arena_device.argtypes = [C.c_void_p]
    lib.pw_batch_arena_device.restype = C.c_void_p
    lib.pw_arena_upload.argtypes = [C.c_int, C.c_void_p, C.c_uint64]
    lib.pw_arena_upload.restype = C.c_void_p
    lib.pw_arena_free.argtypes = [C.c_int, C.c_void_p]
    lib.pw_arena_free.restype = None
    lib.pw_batch_share_arena.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_host_alloc.argtypes = [C.c_uint64]
    lib.pw_host_alloc.restype = C.c_void_p
    lib.pw_host_free.argtypes = [C.c_void_p]
    lib.pw_host_free.restype = None
    lib.pw_batch_upload_arena_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pw_batch_results_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_batch_transcripts_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_batch_solve.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_traceback.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_traceback_from.argtypes = [C.c_void_p, P(C.c_int32), C.c_void_p]
    lib.pw_batch_sync.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_results_device.argtypes = [C.c_void_p]
    lib.pw_batch_results_device.restype = C.c_void_p
    lib.pw_batch_transcripts_device.argtypes = [C.c_void_p]
    lib.pw_batch_transcripts_device.restype = C.c_void_p
    lib.pw_batch_transcripts_bytes.argtypes = [C.c_void_p]
    lib.pw_batch_transcripts_bytes.restype = C.c_uint64
    lib.pw_batch_tx_slot.argtypes = [C.c_void_p, C.c_int32, P(C.c_uint64), P(C.c_int32)]
    lib.pw_batch_results.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_transcripts.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_scores.argtypes = [C.c_void_p, C.c_int32, P(C.c_double), C.c_int64]
    lib.pw_batch_table.argtypes = [C.c_void_p, C.c_int32, P(C.c_double), C.c_int64]
    lib.pw_batch_masks.argtypes = [C.c_void_p, C.c_int32, P(C.c_uint8), C.c_int64]
    lib.pw_batch_fill_ms.argtypes = [C.c_void_p]
    lib.pw_batch_fill_ms.restype = C.c_float
    lib.pw_batch_trace_ms.argtypes = [C.c_void_p]
    lib.pw_batch_trace_ms.restype = C.c_float
    lib.pw_batch_pack_transcripts.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_packed_device.argtypes = [C.c_void_p]
    lib.pw_batch_packed_device.restype = C.c_void_p
    lib.pw_batch_packed_offsets_device.argtypes = [C.c_void_p]
    lib.pw_batch_packed_offsets_device.restype = C.c_void_p
    lib.pw_batch_packed_total_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_batch_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pw_plan_only.argtypes = [P(pw_scoring), C.c_int32, P(pw_pair), C.c_uint64, C.c_uint32, C.c_char_p, C.c_int32, P(C.c_int32)]
    # include/pw_txsum.h
    lib.pw_batch_summarize.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_summaries_device.argtypes = [C.c_void_p]
    lib.pw_batch_summaries_device.restype = C.c_void_p
    lib.pw_batch_summaries_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_batch_summaries.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_tx_summarize_packed.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    # include/pw_cigar.h
    lib.pw_batch_cigars.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pw_batch_cigar_runs_device.argtypes = [C.c_void_p]
    lib.pw_batch_cigar_runs_device.restype = C.c_void_p
    lib.pw_batch_cigar_offsets_device.argtypes = [C.c_void_p]
    lib.pw_batch_cigar_offsets_device.restype = C.c_void_p
    lib.pw_batch_cigar_total.argtypes = [C.c_void_p]
    lib.pw_batch_cigar_total.restype = C.c_uint64
    lib.pw_batch_cigar.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.pw_tx_cigar_packed.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
    # include/pw_pileup.h
    lib.pw_pileup_create.argtypes = [C.c_int, C.c_int64, C.c_int]
    lib.pw_pileup_create.restype = C.c_void_p
    lib.pw_pileup_destroy.argtypes = [C.c_void_p]
    lib.pw_pileup_destroy.restype = None
    lib.pw_pileup_clear.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_batch_pileup_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pw_pileup_counts_device.argtypes = [C.c_void_p]
    lib.pw_pileup_counts_device.restype = C.c_void_p
    lib.pw_pileup_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.pw_pileup_set_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.pw_pileup_call.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.pw_pileup_sites_device.argtypes = [C.c_void_p]
    lib.pw_pileup_sites_device.restype = C.c_void_p
    lib.pw_pileup_sites.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    # include/pw_polish.h
    lib.pw_pileup_create_ins.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int]
    lib.pw_pileup_create_ins.restype = C.c_void_p
    lib.pw_pileup_ins_slots.argtypes = [C.c_void_p]
    lib.pw_pileup_ins_counts_device.argtypes = [C.c_void_p]
    lib.pw_pileup_ins_counts_device.restype = C.c_void_p
    lib.pw_pileup_ins_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.pw_batch_pileup_add_sides.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int64, C.c_void_p]
    lib.pw_pileup_add_letters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p]
    lib.pw_pileup_polish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    lib.pw_pileup_polished_total.argtypes = [C.c_void_p]
    lib.pw_pileup_polished_total.restype = C.c_int64
    lib.pw_pileup_polished_offsets.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_pileup_polished_letters.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_pileup_polished_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_pileup_polished_letters_device.argtypes = [C.c_void_p]
    lib.pw_pileup_polished_letters_device.restype = C.c_void_p
    lib.pw_pileup_polished_offsets_device.argtypes = [C.c_void_p]
    lib.pw_pileup_polished_offsets_device.restype = C.c_void_p
    # include/pw_graph.h
    lib.pw_graph_create.argtypes = [C.c_int, C.c_int64, C.c_void_p]
    lib.pw_graph_create.restype = C.c_void_p
    lib.pw_graph_free.argtypes = [C.c_void_p]
    lib.pw_graph_free.restype = None
    for f in ('pw_graph_num_overlaps', 'pw_graph_device_bytes', 'pw_graph_num_arcs', 'pw_graph_num_unitigs',
              'pw_graph_num_members', 'pw_graph_contig_total'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_int64
    lib.pw_graph_reduce_ms.argtypes = [C.c_void_p]
    lib.pw_graph_reduce_ms.restype = C.c_double
    lib.pw_graph_add_overlaps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_batch_graph_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_graph_build.argtypes = [C.c_void_p, P(pw_graph_params), C.c_void_p]
    lib.pw_graph_build_clean.argtypes = [C.c_void_p, P(pw_graph_params), P(pw_graph_clean_params), C.c_void_p]
    for f in ('pw_graph_overlaps', 'pw_graph_contained', 'pw_graph_dropped', 'pw_graph_arcs', 'pw_graph_rows', 'pw_graph_unitigs', 'pw_graph_members',
              'pw_graph_contig_offsets', 'pw_graph_contig_letters'):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    for f in ('pw_graph_overlaps_device', 'pw_graph_contained_device', 'pw_graph_dropped_device', 'pw_graph_arcs_device', 'pw_graph_rows_device',
              'pw_graph_unitigs_device', 'pw_graph_members_device', 'pw_graph_contig_letters_device', 'pw_graph_contig_offsets_device'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_void_p
    lib.pw_graph_contigs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    # include/pw_consensus.h
    lib.pw_graph_place.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_graph_consensus_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_double, C.c_void_p]
    for f in ('pw_graph_cons_num_tasks', 'pw_graph_cons_num_cols', 'pw_graph_cons_arena_bytes'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_int64
    for f in ('pw_graph_placements', 'pw_graph_cons_cstart', 'pw_graph_cons_tasks'):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    for f in ('pw_graph_placements_device', 'pw_graph_cons_cstart_device', 'pw_graph_cons_tasks_device', 'pw_graph_cons_arena_device'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_void_p
    # include/pw_rounds.h
    lib.pw_pileup_polish_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    lib.pw_pileup_colmap_device.argtypes = [C.c_void_p]
    lib.pw_pileup_colmap_device.restype = C.c_void_p
    lib.pw_pileup_colmap.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.pw_graph_consensus_relayout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_int32, C.c_double, C.c_void_p]
    lib.pw_graph_cons_round.argtypes = [C.c_void_p]
    for f in ('pw_graph_cons_positions', 'pw_graph_cons_lengths'):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p]
    # include/pw_seeds.h
    lib.pw_seeds_create.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                    P(C.c_uint64), C.c_int, C.c_int]
    lib.pw_seeds_create.restype = C.c_void_p
    lib.pw_seeds_build.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.pw_seeds_num_rows.argtypes = [C.c_void_p]
    lib.pw_seeds_num_rows.restype = C.c_int64
    lib.pw_seeds_is_self.argtypes = [C.c_void_p]
    lib.pw_seeds_rows_device.argtypes = [C.c_void_p]
    lib.pw_seeds_rows_device.restype = C.c_void_p
    lib.pw_seeds_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_seeds_count.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_int32, C.c_int32]
    lib.pw_seeds_count.restype = C.c_int64
    lib.pw_seeds_kmers.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    lib.pw_seeds_kmers.restype = C.c_int64
    lib.pw_seeds_band_neighbours.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.pw_seeds_graph_build.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.pw_seeds_graph_build.restype = C.c_int64
    lib.pw_seeds_graph_num_points.argtypes = [C.c_void_p]
    lib.pw_seeds_graph_num_points.restype = C.c_int64
    lib.pw_seeds_graph_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_seeds_graph_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_seeds_graph_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_seeds_graph_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_seeds_build_ms.argtypes = [C.c_void_p]
    lib.pw_seeds_build_ms.restype = C.c_double
    lib.pw_seeds_algorithmic_bytes.argtypes = [C.c_void_p]
    lib.pw_seeds_algorithmic_bytes.restype = C.c_int64
    lib.pw_seeds_destroy.argtypes = [C.c_void_p]
    lib.pw_seeds_destroy.restype = None
    lib.pw_seeds_last_error.restype = C.c_char_p
    # include/pw_mseeds.h
    lib.pw_mseeds_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.pw_mseeds_create.restype = C.c_void_p
    lib.pw_mseeds_build.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.pw_mseeds_num_seqs.argtypes = [C.c_void_p]
    lib.pw_mseeds_num_rows.argtypes = [C.c_void_p]
    lib.pw_mseeds_num_rows.restype = C.c_int64
    lib.pw_mseeds_rows_device.argtypes = [C.c_void_p]
    lib.pw_mseeds_rows_device.restype = C.c_void_p
    lib.pw_mseeds_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_mseeds_count_many.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_mseeds_graph_build.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.pw_mseeds_graph_build.restype = C.c_int64
    lib.pw_mseeds_graph_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_mseeds_graph_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_mseeds_graph_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in ('pw_mseeds_build_ms', 'pw_mseeds_graph_ms', 'pw_mseeds_components_ms', 'pw_mseeds_count_ms'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_double
    lib.pw_mseeds_algorithmic_bytes.argtypes = [C.c_void_p]
    lib.pw_mseeds_algorithmic_bytes.restype = C.c_int64
    lib.pw_mseeds_destroy.argtypes = [C.c_void_p]
    lib.pw_mseeds_destroy.restype = None
    lib.pw_mseeds_last_error.restype = C.c_char_p
    # include/pw_qseeds.h
    lib.pw_qseeds_create.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int]
    lib.pw_qseeds_create.restype = C.c_void_p
    lib.pw_qseeds_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_void_p]
    lib.pw_qseeds_build_stranded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.pw_qseeds_num_queries.argtypes = [C.c_void_p]
    lib.pw_qseeds_num_queries.restype = C.c_int64
    lib.pw_qseeds_num_rows.argtypes = [C.c_void_p]
    lib.pw_qseeds_num_rows.restype = C.c_int64
    lib.pw_qseeds_rows_device.argtypes = [C.c_void_p]
    lib.pw_qseeds_rows_device.restype = C.c_void_p
    lib.pw_qseeds_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_qseeds_row_offsets.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_qseeds_count_boxes.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    lib.pw_qseeds_graph_build.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.pw_qseeds_graph_build.restype = C.c_int64
    lib.pw_qseeds_graph_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_qseeds_graph_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_qseeds_graph_components.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in ('pw_qseeds_build_ms', 'pw_qseeds_graph_ms', 'pw_qseeds_components_ms', 'pw_qseeds_count_ms'):
        getattr(lib, f).argtypes = [C.c_void_p]
        getattr(lib, f).restype = C.c_double
    lib.pw_qseeds_components_rounds.argtypes = [C.c_void_p]
    lib.pw_qseeds_destroy.argtypes = [C.c_void_p]
    lib.pw_qseeds_destroy.restype = None
    lib.pw_qseeds_last_error.restype = C.c_char_p
    # include/pw_overlap.h
    lib.pw_overlap_bands.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                     C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.pw_overlap_all_pairs.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.pw_overlap_bands_stranded.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                              C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_overlap_all_pairs_stranded.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                                  C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pw_overlap_all_pairs_capped.argtypes = lib.pw_overlap_all_pairs_stranded.argtypes + [C.c_uint32, P(pw_overlap_cap_stats)]
    lib.pw_overlap_all_pairs_sampled.argtypes = lib.pw_overlap_all_pairs_capped.argtypes + [C.c_int, P(pw_overlap_sample_stats)]
    lib.pw_overlap_arena_upload.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int]
    lib.pw_overlap_arena_upload.restype = C.c_void_p
    lib.pw_overlap_arena_read.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.pw_overlap_last_ms.restype = C.c_double
    lib.pw_overlap_last_error.restype = C.c_char_p
    # include/pw_kmers.h
    lib.pw_kmers_create.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.pw_kmers_create.restype = C.c_void_p
    lib.pw_kmers_build.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    lib.pw_kmers_build_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int,
                                           C.c_void_p]
    lib.pw_kmers_num_positions.argtypes = [C.c_void_p]
    lib.pw_kmers_num_positions.restype = C.c_int64
    lib.pw_kmers_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_kmers_read_starts.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_kmers_num_entries.argtypes = [C.c_void_p]
    lib.pw_kmers_num_entries.restype = C.c_int64
    lib.pw_kmers_num_distinct.argtypes = [C.c_void_p]
    lib.pw_kmers_num_distinct.restype = C.c_int64
    lib.pw_kmers_distinct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.pw_kmers_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pw_kmers_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.pw_kmers_spectrum.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pw_kmers_occurrences.argtypes = [C.c_void_p, C.c_void_p]
    lib.pw_kmers_destroy.argtypes = [C.c_void_p]
    lib.pw_kmers_destroy.restype = None
    lib.pw_kmers_last_ms.restype = C.c_double
    lib.pw_kmers_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def last_error():
    return (load().pw_last_error() or b'').decode('utf-8', 'replace')
