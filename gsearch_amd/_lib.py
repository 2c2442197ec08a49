"""ctypes binding of libgsearch_amd.so (the C ABI declared in include/gsearch_amd.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is visible, calls fail loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("GS_LIB_PATH") or os.path.join(_HERE, "libgsearch_amd.so")      # GS_LIB_PATH: A/B builds (tools/ only)

GS_OK, GS_ERR_INVALID, GS_ERR_HIP, GS_ERR_UNSUPPORTED, GS_ERR_STATE, GS_ERR_IO = 0, -1, -2, -3, -4, -5
ALGO = {"prob": 0, "super": 1, "super2": 2, "hll": 3, "optdens": 4, "revoptdens": 5, "hmh": 6}   # hmh: HyperMinHash of hypermash (SPEC 7)
HMH_REGISTERS = 16384
DATA = {"dna": 0, "aa": 1, "dna_fwd": 2}   # dna_fwd: forward window, no reverse-complement minimum (bindash.rs:346-354, k <= 14)
KIND_U16, KIND_U32, KIND_U64, KIND_F32 = 0, 1, 2, 3


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gsearch_amd error %d: %s" % (code, msg))
        self.code = code


class SketchParams(C.Structure):
    """kmerutils::sketcharg::SeqSketcherParams {kmer_size, sketch_size, algo, data_t}"""
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("algo", C.c_uint32), ("data_t", C.c_uint32)]


class IndexParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("m", C.c_uint32), ("max_nb_conn", C.c_uint32), ("capacity", C.c_uint64),
                ("max_layer", C.c_uint32), ("ef_construction", C.c_uint32), ("scale_modify", C.c_double),
                ("extend_candidates", C.c_int), ("keep_pruned", C.c_int), ("seed", C.c_uint64),
                ("insert_batch", C.c_uint32)]


class EmbedParamsC(C.Structure):
    """gs_embed_params (SPEC 8)"""
    _fields_ = [("dim", C.c_uint32), ("epochs", C.c_uint32), ("neg_samples", C.c_uint32), ("neg_rate", C.c_float), ("lr", C.c_float),
                ("seed", C.c_uint64)]


class KnnStatsC(C.Structure):
    """gs_knn_stats (SPEC 8)"""
    _fields_ = [("n", C.c_uint64), ("n_edges", C.c_uint64), ("n_empty", C.c_uint64), ("knbn", C.c_uint32), ("max_occ", C.c_uint32),
                ("occ_mean", C.c_double), ("occ_std", C.c_double), ("occ_skew", C.c_double), ("hub_ids", C.c_uint64 * 16),
                ("hub_occ", C.c_uint32 * 16), ("q_first", C.c_float * 7), ("q_last", C.c_float * 7)]


class EmbedQualityC(C.Structure):
    """gs_embed_quality_summary (SPEC 8.1)"""
    _fields_ = [("n", C.c_uint64), ("n_rows", C.c_uint64), ("n_edges", C.c_uint64), ("n_conserved", C.c_uint64), ("n_nomatch", C.c_uint64),
                ("knbn", C.c_uint32), ("kq_eff", C.c_uint32), ("mean_conserved", C.c_double), ("frac_conserved", C.c_double),
                ("q_edge", C.c_double * 7), ("q_radius", C.c_double * 7), ("q_ratio", C.c_double * 7)]


class ClusterParamsC(C.Structure):
    """gs_cluster_params (SPEC 10)"""
    _fields_ = [("n_cluster", C.c_uint32), ("fraction", C.c_double), ("max_iter", C.c_uint32), ("seed", C.c_uint64)]


class ClusterInfoC(C.Structure):
    """gs_cluster_info (SPEC 10)"""
    _fields_ = [("n_core", C.c_uint64), ("iterations", C.c_uint32), ("converged", C.c_uint32), ("cost_core", C.c_uint64), ("cost_all", C.c_uint64)]


class DerepInfoC(C.Structure):
    """gs_derep_info (SPEC 18)"""
    _fields_ = [("n_clusters", C.c_uint64), ("n_singletons", C.c_uint64), ("largest", C.c_uint64), ("c_max", C.c_uint32), ("reserved", C.c_uint32)]


class BigsiParamsC(C.Structure):
    """gs_bigsi_params (SPEC 11)"""
    _fields_ = [("k", C.c_uint32), ("num_hash", C.c_uint32), ("bloom_size", C.c_uint64), ("data_t", C.c_uint32), ("minimizer", C.c_uint32),
                ("coverage_filter", C.c_uint32)]


class BigsiDescC(C.Structure):
    """gs_bigsi_desc (SPEC 11)"""
    _fields_ = [("prm", BigsiParamsC), ("n_colours", C.c_uint64), ("colour_capacity", C.c_uint64), ("row_words", C.c_uint64)]


class HnswrsDescriptionC(C.Structure):
    """gs_hnswrs_description (SPEC 16.1)"""
    _fields_ = [("dump_mode", C.c_uint32), ("max_nb_conn", C.c_uint32), ("nb_layer", C.c_uint32), ("kind", C.c_int32), ("ef", C.c_uint64), ("nb_point", C.c_uint64),
                ("dimension", C.c_uint64), ("distance", C.c_char * 128), ("t_name", C.c_char * 32), ("n_upper", C.c_uint64), ("entry", C.c_uint64),
                ("ids_are_nodes", C.c_uint64), ("digest", C.c_uint64)]


class BigsiFileDescriptionC(C.Structure):
    """gs_bigsi_file_description (SPEC 16.2)"""
    _fields_ = [("version", C.c_uint32), ("k", C.c_uint32), ("num_hash", C.c_uint32), ("data_t", C.c_uint32), ("minimizer_len", C.c_uint32),
                ("has_accessions", C.c_uint32), ("bloom_size", C.c_uint64), ("n_colours", C.c_uint64), ("row_words", C.c_uint64), ("digest", C.c_uint64)]


class HmmInfoC(C.Structure):
    """gs_hmm_info (SPEC 13)"""
    _fields_ = [("name", C.c_char * 64), ("acc", C.c_char * 32), ("M", C.c_uint32), ("flags", C.c_uint32), ("ga", C.c_double * 2), ("tc", C.c_double * 2),
                ("nc", C.c_double * 2), ("mu", C.c_double), ("lam", C.c_double), ("ga_units", C.c_int32), ("tbm", C.c_int32)]


class OrfParamsC(C.Structure):
    """gs_orf_params (SPEC 14)"""
    _fields_ = [("min_aa", C.c_uint32), ("max_aa", C.c_uint32), ("table", C.c_uint32), ("flags", C.c_uint32)]


ORF_TILE, ORF_MIN_AA = 192, 30


class GeneParamsC(C.Structure):
    """gs_gene_params (SPEC 15)"""
    _fields_ = [("min_aa", C.c_uint32), ("table", C.c_uint32), ("train_min_aa", C.c_uint32), ("min_train_codons", C.c_uint32), ("min_score", C.c_int32),
                ("max_overlap", C.c_uint32), ("rounds", C.c_uint32), ("flags", C.c_uint32)]


GENE_STRAND, GENE_TYPE_SHIFT, GENE_TYPE_EDGE, GENE_OPEN3, GENE_HAS_START, GENE_CANDIDATE, GENE_OPEN5 = 1, 1, 3, 8, 16, 32, 64
GENE_NO_START, GENE_TRAINED = 0xFFFFFFFFFFFFFFFF, 1

HMM_MAX_M, HMM_MAX_L, HMM_NO_SCORE, HMM_NO_HIT, HMM_TABLE_ROWS = 1280, 1 << 18, -(1 << 31), 0xFFFFFFFF, 27
HMM_AA = "ACDEFGHIKLMNPQRSTVWY"                     # the residues in the order of a table's 20 match rows (gs_hmm_parse_mem)
HMM_HAS_GA, HMM_HAS_TC, HMM_HAS_NC, HMM_HAS_STATS = 1, 2, 4, 8
HMM_FWD_MAX_L, HMM_LSE_N, HMM_FLOOR_ALL = 65536, 5903, -(1 << 31) + 1
HMM_VF_OVER = (1 << 31) - 1                         # vf of a record whose int16 cells overflow (SPEC 13.7): above every floor
HMM_TRACE_MAX_L, HMM_DOM_WORDS = 65536, 8
HMM_ENV_WORDS, HMM_ENV_LO, HMM_ENV_HI = 4, -156, -425
HMM_N2_WORDS, HMM_N2_OMEGA = 4, -8192              # SPEC 13.5: corr, dom_bias, seg_raw, mass; 1024 log2(1 / 256)
HMM_ALI_WORDS, HMM_ALI_MAX_LD, HMM_EXP2_N = 8, 8192, 1024      # SPEC 13.6: i_from, i_to, k_from, k_to, oa, n_match, n_ins, n_del

EMBED_HIST_BINS = 64
EMBED_QUANTILES = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
EMBQ_TIMES = 20                                     # GS_EMBQ_TIMES: edge pass, rank pass, 16 radius passes, rank finish, summary on the host

# every symbol include/gsearch_amd.h declares: name -> (restype, argtypes)
_vp, _u64, _u32, _i = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
_PP = C.POINTER(SketchParams)
SYMBOLS = {
    "gs_last_error": (C.c_char_p, []),
    "gs_version": (C.c_char_p, []),
    "gs_ctx_create": (_i, [C.POINTER(_vp), _i, _vp]),
    "gs_ctx_destroy": (None, [_vp]),
    "gs_ctx_sync": (_i, [_vp]),
    "gs_ctx_release_scratch": (_i, [_vp]),
    "gs_ctx_stream": (_vp, [_vp]),
    "gs_ctx_device_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_u64), C.c_char_p, C.c_size_t]),
    "gs_ctx_last_sketch_info": (_i, [_vp, _vp]),
    "gs_ctx_timer_start": (_i, [_vp]),
    "gs_ctx_timer_stop": (_i, [_vp, C.POINTER(C.c_float)]),
    "gs_ctx_profile": (_i, [_vp, _i]),
    "gs_ctx_profile_read": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(_u64), _i]),
    "gs_dev_alloc": (_i, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "gs_dev_free": (_i, [_vp, _vp]),
    "gs_dev_upload": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "gs_dev_download": (_i, [_vp, _vp, _vp, C.c_size_t]),
    "gs_dev_memset": (_i, [_vp, _vp, _i, C.c_size_t]),
    "gs_check_params": (_i, [_PP]),
    "gs_sig_kind": (_i, [_PP]),
    "gs_sig_elem_bytes": (C.c_size_t, [_PP]),
    "gs_value_bits": (_i, [_PP]),
    "gs_sketch_batch": (_i, [_vp, _PP, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp]),
    "gs_sketch_batch_dev": (_i, [_vp, _PP, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp]),
    "gs_fasta_scan": (_i, [_vp, _u64, _i, _u64, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "gs_pack_fasta_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_filter_aa_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_is_fasta_file": (_i, [C.c_char_p, _i]),
    "gs_read_fasta_file": (_i, [C.c_char_p, C.POINTER(_vp), C.POINTER(_u64)]),
    "gs_host_free": (None, [_vp]),
    "gs_list_fasta_files": (_i, [C.c_char_p, _i, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gs_sketch_files": (_i, [_vp, _PP, C.POINTER(C.c_char_p), _u64, _i, _u32, _u32, _vp, _vp, _vp, _vp]),
    "gs_sketch_files_ex": (_i, [_vp, _PP, C.POINTER(C.c_char_p), _u64, _i, _u32, _u32, _vp, _vp, _vp, _vp, _u32]),
    "gs_gunzip_batch": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "gs_pack_dna": (_u64, [_vp, _u64, _vp, _u64]),
    "gs_filter_aa": (_u64, [_vp, _u64, _vp]),
    "gs_hamming_qxc": (_i, [_vp, _i, _u32, _vp, _u64, _vp, _u64, _vp]),
    "gs_hamming_qxc_dev": (_i, [_vp, _i, _u32, _vp, _u64, _vp, _u64, _vp]),
    "gs_hamming_pairs": (_i, [_vp, _i, _u32, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp]),
    "gs_ani": (C.c_double, [C.c_double, _i, _i]),
    "gs_hmh_cardinality": (_i, [_vp, _vp, _u64, _vp]),
    "gs_hmh_cardinality_dev": (_i, [_vp, _vp, _u64, _vp]),
    "gs_hmh_similarity_qxc": (_i, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "gs_hmh_similarity_qxc_dev": (_i, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "gs_hmh_distance": (C.c_double, [C.c_double, _i]),
    "gs_fastq_scan": (_i, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "gs_hmh_sketch_files": (_i, [_vp, _u32, C.POINTER(C.c_char_p), _u64, _u32, _vp, _vp, _vp, _vp]),
    # superaai (SPEC 9)
    "gs_frac_max_hash": (_u64, [_u32]),
    "gs_frac_sketch_batch": (_i, [_vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _u64, C.POINTER(C.POINTER(_u64)), _vp]),
    "gs_frac_sketch_batch_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp]),
    "gs_frac_similarity_qxc": (_i, [_vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_frac_similarity_qxc_dev": (_i, [_vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_frac_sketch_files": (_i, [_vp, _u32, _u32, _u32, C.POINTER(C.c_char_p), _u64, _u32, C.POINTER(C.POINTER(_u64)), _vp, _vp, _vp, _vp]),
    "gs_aai": (C.c_double, [C.c_double, _u32]),
    "gs_superaai_write": (_i, [C.c_char_p, C.POINTER(C.c_char_p), _u64, C.POINTER(C.c_char_p), _u64, _vp, _u32]),
    # superani (SPEC 12)
    "gs_ani_sketch_batch": (_i, [_vp, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _u64, C.POINTER(C.POINTER(_u32)), _vp]),
    "gs_ani_sketch_batch_dev": (_i, [_vp, _u32, _u32, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp]),
    "gs_ani_pairs": (_i, [_vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "gs_ani_pairs_dev": (_i, [_vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "gs_ani_chain_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_ani_estimate": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    # hmmsearch (SPEC 13)
    "gs_hmm_parse_mem": (_i, [_vp, _u64, _u32, C.POINTER(HmmInfoC), _vp, _u64, C.POINTER(_u32)]),
    "gs_hmm_specials": (_i, [_u64, _u32, _vp]),
    "gs_hmm_db_load": (_i, [_vp, C.POINTER(C.c_char_p), _u64, C.POINTER(_vp)]),
    "gs_hmm_db_load_mem": (_i, [_vp, C.POINTER(_vp), C.POINTER(_u64), _u64, C.POINTER(_vp)]),
    "gs_hmm_db_free": (None, [_vp]),
    "gs_hmm_db_info": (_i, [_vp, C.POINTER(_u64), C.POINTER(HmmInfoC), _u64]),
    "gs_hmm_db_tables": (_i, [_vp, _u64, _vp, _u64]),
    "gs_hmm_db_consensus": (_i, [_vp, _u64, _vp, _u64]),
    "gs_hmm_search_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_search": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_best_hits_dev": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "gs_hmm_bits": (C.c_double, [C.c_int32]),
    "gs_hmm_evalue": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_double]),
    "gs_hmm_logsum_table": (_i, [_vp, _u64]),
    "gs_hmm_parse_stats_mem": (_i, [_vp, _u64, _u32, _vp, C.POINTER(_u32)]),
    "gs_hmm_viterbi_floor": (_i, [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int32)]),
    "gs_hmm_search_forward_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_hmm_search_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_hmm_forward_evalue": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_double]),
    "gs_hmm_search_msv_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_search_msv": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_search_filtered_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_search_filtered": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_search_vit16_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_search_vit16": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "gs_hmm_db_tables16": (_i, [_vp, _u64, _vp, _u64]),
    "gs_hmm_search_staged_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_search_staged": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_trace": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp]),
    "gs_hmm_trace_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp]),
    "gs_hmm_envelopes": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_envelopes_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_null2": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_null2_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_exp2_table": (_i, [_vp, _u64]),
    "gs_hmm_align": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_align_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_hit_records_dev": (_i, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "gs_hmm_hit_records": (_i, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    # orfs (SPEC 14)
    "gs_orf_codon_table": (_i, [_u32, C.c_char_p]),
    "gs_orf_translate_dev": (_i, [_vp, C.POINTER(OrfParamsC), _vp, _u64, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "gs_orf_translate": (_i, [_vp, C.POINTER(OrfParamsC), _vp, _u64, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    # genes (SPEC 15)
    "gs_gene_params_default": (GeneParamsC, []),
    "gs_gene_log2_q16": (_u32, [_u64]),
    "gs_gene_train_dev": (_i, [_vp, C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "gs_gene_train_host": (_i, [C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "gs_gene_score_dev": (_i, [_vp, C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_gene_score_host": (_i, [C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_gene_call_dev": (_i, [_vp, C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "gs_gene_call": (_i, [_vp, C.POINTER(GeneParamsC), _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "gs_index_create": (_i, [_vp, C.POINTER(IndexParams), C.POINTER(_vp)]),
    "gs_index_destroy": (None, [_vp]),
    "gs_index_nb_point": (_u64, [_vp]),
    "gs_index_get_params": (_i, [_vp, C.POINTER(IndexParams)]),
    "gs_index_parallel_insert": (_i, [_vp, _vp, _u64]),
    "gs_index_parallel_insert_dev": (_i, [_vp, _vp, _u64]),
    "gs_index_parallel_insert_ids": (_i, [_vp, _vp, _vp, _u64]),
    "gs_index_parallel_insert_ids_dev": (_i, [_vp, _vp, _vp, _u64]),
    "gs_index_sketch_and_search_dev": (_i, [_vp, _PP, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "gs_index_set_ids": (_i, [_vp, _vp, _u64]),
    "gs_index_get_ids": (_i, [_vp, _u64, _u64, _vp]),
    "gs_index_parallel_search_pid": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_index_parallel_search_pid_dev": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_index_parallel_search": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp]),
    "gs_index_parallel_search_dev": (_i, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp]),
    "gs_index_count_matrix": (_i, [_vp, _vp, _u64, _vp]),
    "gs_index_bruteforce_search": (_i, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "gs_index_exact_search": (_i, [_vp, _vp, _u64, _u32, C.c_float, _vp, _vp, _vp]),
    "gs_index_exact_search_dev": (_i, [_vp, _vp, _u64, _u32, C.c_float, _vp, _vp, _vp]),
    "gs_index_knn_graph": (_i, [_vp, _u32, C.c_float, _u64, _u64, _vp, _vp, _vp]),
    "gs_index_knn_graph_dev": (_i, [_vp, _u32, C.c_float, _u64, _u64, _vp, _vp, _vp]),
    "gs_embed_params_default": (EmbedParamsC, []),
    "gs_embed_knn_graph": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(EmbedParamsC), _vp, _vp, _vp]),
    "gs_embed_knn_graph_dev": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(EmbedParamsC), _vp, _vp, _vp]),
    "gs_index_embed": (_i, [_vp, _u32, C.c_float, C.POINTER(EmbedParamsC), _vp, _vp]),
    "gs_knn_graph_stats": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(KnnStatsC), _vp, _vp]),
    "gs_index_knn_graph_stats": (_i, [_vp, _u32, C.c_float, C.POINTER(KnnStatsC), _vp, _vp]),
    "gs_embed_quality": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, _vp, _u32, _u32, C.POINTER(EmbedQualityC), _vp, _vp, _vp, _vp]),
    "gs_embed_quality_dev": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "gs_index_embed_quality": (_i, [_vp, _u32, C.c_float, _vp, _u32, _u32, C.POINTER(EmbedQualityC), _vp, _vp, _vp, _vp]),
    "gs_embed_quality_last_ms": (_i, [_vp, _vp]),
    # hnswcore (SPEC 10)
    "gs_cluster_params_default": (ClusterParamsC, []),
    "gs_index_nearest_of": (_i, [_vp, _vp, _u64, _vp, _vp]),
    "gs_index_cluster": (_i, [_vp, C.POINTER(ClusterParamsC), _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(ClusterInfoC)]),
    "gs_index_components": (_i, [_vp, C.c_float, _vp, C.POINTER(DerepInfoC)]),
    "gs_index_derep": (_i, [_vp, C.c_float, _vp, _vp, _vp, C.POINTER(DerepInfoC)]),
    # bigsig (SPEC 11)
    "gs_bigsi_check_params": (_i, [C.POINTER(BigsiParamsC)]),
    "gs_bigsi_create": (_i, [_vp, C.POINTER(BigsiParamsC), _u64, C.POINTER(_vp)]),
    "gs_bigsi_create_mini": (_i, [_vp, C.POINTER(BigsiParamsC), _u32, _u64, C.POINTER(_vp)]),
    "gs_bigsi_minimizer_len": (_u32, [_vp]),
    "gs_bigsi_add_batch_min_count_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32]),
    "gs_bigsi_add_batch_min_count": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _u64, _u32]),
    "gs_bigsi_minimizers": (_i, [_vp, _vp, _u64, _u32, _u32, _u32, _u32, _u64, _vp, _vp, C.POINTER(_u64)]),
    "gs_bigsi_free": (None, [_vp]),
    "gs_bigsi_info": (_i, [_vp, C.POINTER(BigsiDescC)]),
    "gs_bigsi_add_batch_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "gs_bigsi_add_batch": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _u64]),
    "gs_bigsi_bits_set": (_i, [_vp, _u64, _u64, _vp, _vp]),
    "gs_bigsi_rows": (_i, [_vp, _vp, _u64, _vp]),
    "gs_bigsi_query_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    "gs_bigsi_query": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    "gs_bigsi_classify_dev": (_i, [_vp, _u64, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    "gs_bigsi_set_accessions": (_i, [_vp, C.POINTER(C.c_char_p), _u64]),
    "gs_bigsi_accessions": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "gs_bigsi_save": (_i, [_vp, C.c_char_p]),
    "gs_bigsi_load": (_i, [_vp, C.c_char_p, _u64, C.POINTER(_vp)]),
    "gs_bigsi_describe": (_i, [C.c_char_p, C.POINTER(BigsiFileDescriptionC)]),
    "gs_bigsi_verify": (_i, [C.c_char_p, C.POINTER(BigsiFileDescriptionC)]),
    "gs_bigsi_positions": (_i, [_u64, _u32, _u64, _vp]),
    "gs_bigsi_split": (_i, [_vp, _vp, _u64, _u32, _u64, _u64, _vp, _vp, C.POINTER(_u64)]),
    "gs_bigsi_tail": (C.c_double, [_u64, _u64, _u32, _u32, _u32]),
    "gs_bigsig_write_reads": (_i, [C.c_char_p, C.POINTER(C.c_char_p), _u64, C.POINTER(C.c_char_p), _u64, _vp, _vp, _vp, _vp]),
    # bigsig, tied top hits and the six-field report (SPEC 11.2)
    "gs_bigsi_query_ties_dev": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "gs_bigsi_query_ties": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "gs_bigsi_verdict_dev": (_i, [_vp, _u64, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    "gs_bigsi_verdict_code": (_u32, [_u32, _u32, _u32, C.c_double, C.c_double]),
    "gs_bigsig_write_report": (_i, [C.c_char_p, C.POINTER(C.c_char_p), _u64, C.POINTER(C.c_char_p), _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    "gs_index_import": (_i, [_vp, _vp, _u64, _vp, C.c_int64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_index_export": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gs_index_get_data": (_i, [_vp, _u64, _u64, _vp]),
    "gs_index_save": (_i, [_vp, C.c_char_p]),
    "gs_index_load": (_i, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "gs_index_dump_hnswrs": (_i, [_vp, C.c_char_p]),
    "gs_index_dump_hnswrs_ex": (_i, [_vp, C.c_char_p, _u32]),
    "gs_index_load_hnswrs": (_i, [_vp, C.c_char_p, C.POINTER(IndexParams), C.POINTER(_vp)]),
    "gs_hnswrs_describe": (_i, [C.c_char_p, C.POINTER(HnswrsDescriptionC)]),
    "gs_hnswrs_verify": (_i, [C.c_char_p, C.POINTER(HnswrsDescriptionC)]),
    "gs_index_insert_evals": (_u64, [_vp]),
    "gs_index_search_stats": (_i, [_vp, _vp, _i]),
    "gs_comm_unique_id": (_i, [_vp]),
    "gs_comm_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "gs_comm_destroy": (None, [_vp]),
    "gs_comm_rank": (_i, [_vp]),
    "gs_comm_size": (_i, [_vp]),
    "gs_comm_allgather_topk_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "gs_comm_allgatherv_topk_dev": (_i, [_vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _vp]),
    "gs_comm_allgatherv_topk_async_dev": (_i, [_vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _vp]),
    "gs_comm_wait": (_i, [_vp, _vp]),
    "gs_index_release_build_scratch": (_i, [_vp]),
    "gs_topk_block_bytes": (_u64, [_u64, _u32]),
    "gs_topk_pack": (_i, [_vp, _vp, _u64, _u64, _u32, _vp]),
    "gs_topk_unpack": (_i, [_vp, _i, _u64, _u32, _vp, _vp, _vp]),
    "gs_topk_merge_dev": (_i, [_vp, _vp, _vp, _u32, _u64, _u32, _vp, _u32, _vp, _vp]),
    # split databases (SPEC 17 items 12-18)
    "gs_topk_reset_dev": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    "gs_index_search_merge_dev": (_i, [_vp, _vp, _u64, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _vp]),
    "gs_index_search_merge": (_i, [_vp, _vp, _u64, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp, _vp]),
    "gs_synth_dna_dev": (_i, [_vp, _u64, _u64, _u64, _u64, _vp]),
    "gs_synth_aa_dev": (_i, [_vp, _u64, _u64, _u64, _u64, _vp]),
    "gs_synth_dna_family_dev": (_i, [_vp, _u64, _u64, _u64, _u64, _u64, C.c_double, C.c_double, _vp]),
    "gs_synth_sigs_dev": (_i, [_vp, _i, _u32, _u64, _u64, _u64, _u64, C.c_double, C.c_double, _vp]),
    "gs_synth_sigs_skew_dev": (_i, [_vp, _i, _u32, _u64, _u64, _u64, _u64, C.c_double, C.c_double, C.c_double, _vp]),
    "gs_synth_dna_family_skew_dev": (_i, [_vp, _u64, _u64, _u64, _u64, _u64, C.c_double, C.c_double, C.c_double, _vp]),
    # debugging
    "gs_debug_mem_fill": (_i, [_i]),
    "gs_index_debug_fill_scratch": (_i, [_vp, _i]),
    "gs_debug_radix_sort_u64": (_i, [_vp, _vp, _u64, _i, _vp]),
    "gs_debug_run_lengths_u64": (_i, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "gs_debug_scan_u32": (_i, [_vp, _vp, _u64, _vp, _vp]),
    "gs_debug_hamming_strided": (_i, [_vp, _i, _u32, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _i, _vp, _u64, _vp]),
    "gs_debug_hamming_blocks": (_i, [_vp, _i, _u32, _vp, _u64, _u64, _vp, _u64, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _u32, _vp, _u64, _vp]),
}

_lib = None


def load():
    """Load the HIP shared library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError("gsearch_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C gsearch_amd/csrc`. There is no CPU fallback." % SO_PATH)
        L = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)          # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != GS_OK:
        raise GsError(rc, load().gs_last_error().decode("utf-8", "replace"))
    return rc
