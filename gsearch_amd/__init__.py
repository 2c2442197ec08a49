"""gsearch_amd — MI355X-native (gfx950) sketch-and-query hot path of gsearch behind a C ABI.

See DESIGN.md / SPEC.md / INTEGRATION.md. Importing the package does not need a GPU; the first call
that touches the device does, and fails loudly otherwise (no CPU fallback).
"""
from ._lib import ALGO, DATA, GsError, SO_PATH, SYMBOLS, load  # noqa: F401
from .api import (Comm, Context, DistHamming, Hnsw, HyperLogLogSketch, HyperMinHashSketch, Neighbour, OptDensHashSketch, ProbHash3aSketch,  # noqa: F401
                  RevOptDensHashSketch, ReqAnswer, SeqSketcherParams, SuperHash2Sketch, SuperHashSketch, ani, bindash_distance, bindash_sketch_params,
                  debug_hamming_blocks, debug_hamming_strided, debug_mem_fill, debug_radix_sort, debug_run_lengths, debug_scan, default_context, dump_knn_graph, fasta_scan, filter_aa_records, is_fasta_file, list_fasta_files, gunzip_batch, read_fasta_file, pack_dna_records, sketch_fasta_files, sketcher_for, topk_block_bytes, topk_merge_dev, topk_pack, topk_reset_dev, topk_unpack)
from .api import (fastq_scan, hmh_cardinality, hmh_cardinality_dev, hmh_similarity_qxc, hmh_similarity_qxc_dev, hypermash, hypermash_distance,  # noqa: F401
                  read_path_list, write_hypermash_tsv)
from .api import EmbedParams, ann, embed_knn_graph, embed_knn_graph_dev, knn_graph_stats, write_embedding_csv  # noqa: F401
from .api import EMBQ_TILE_P, EMBQ_TILE_Q, embed_quality, embed_quality_dev, embed_quality_last_ms, embed_quality_text  # noqa: F401
from .api import FracMinHashSketch, aai, frac_max_hash, frac_similarity_qxc, frac_similarity_qxc_dev, read_list_lines, superaai, write_superaai  # noqa: F401
from .api import ClusterResult, hnswcore, write_cluster_csv  # noqa: F401
from .api import ComponentsResult, DerepResult, ani_cut  # noqa: F401
from .api import hnswrs_describe, hnswrs_verify  # noqa: F401
from .api import BIGSI_MINI_TILE, Bigsi, bigsi_minimizers, bigsi_positions, bigsi_split, bigsi_tail, bigsig_construct, bigsig_identify, bigsig_write_reads, read_ref_list  # noqa: F401
from .api import BIGSI_VERDICTS, bigsi_verdict_code, bigsig_write_report  # noqa: F401
from .api import AniGenome, AniSketcher, ani_estimate, ani_pairs, superani, write_superani  # noqa: F401
from .api import HmmDb, hmm_bits, hmm_evalue, hmm_parse, hmm_specials, hmm_threshold_units, hmmsearch, universal_genes  # noqa: F401
from .api import UNIVERSAL_STAGES, hit_records, hit_records_dev, universal_sketch  # noqa: F401
from .api import hmm_exp2_table, hmm_forward_evalue, hmm_logsum_table, hmm_parse_stats, hmm_viterbi_floor  # noqa: F401
from .api import ORF_DTYPE, ORF_TILE, orf_codon_table, orf_translate, orf_translate_dev, orf_translate_packed, write_orf_faa  # noqa: F401
from .api import (GENE_DTYPE, GENE_INTERVAL_DTYPE, GENE_START_TYPES, gene_call, gene_call_dev, gene_call_packed, gene_log2_q16, gene_params, gene_score,  # noqa: F401
                  gene_train, genecall, write_gene_faa, write_gene_ffn, write_gene_gff)
from .commands import add, derep, derep_clusters_text, derep_representatives_text, matches_text, reformat, reformat_text, request, rust_display_f64, rust_upper_exp, tohnsw  # noqa: F401
from .split import request_split, split_json_text, tohnsw_split  # noqa: F401
