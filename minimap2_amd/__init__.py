"""minimap2_amd -- MI355X-native seed-chain-extend engine behind minimap2's API.

This package is a thin ctypes mirror of the C ABI in include/mm2amd.h, shaped like the reference's own Python
binding (python/mappy.pyx: Aligner(seq=..., preset=...).map(...)).  All compute happens in libmm2amd.so
(hand-written HIP for gfx950).  There is no CPU fallback: if the library is not built or no GPU is visible,
calls raise Mm2AmdError."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmm2amd.so")


class Mm2AmdError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------------
# struct mirrors (layouts: minimap2_amd/csrc/abi_ref.hpp, checked against the reference headers in tests/)
# ---------------------------------------------------------------------------------------------------------
class KswJob(C.Structure):  # mm2amd_ksw_job_t
    _fields_ = [("query", C.c_void_p), ("target", C.c_void_p), ("qlen", C.c_int32), ("tlen", C.c_int32), ("w", C.c_int32),
                ("zdrop", C.c_int32), ("end_bonus", C.c_int32), ("flag", C.c_int32)]


class FinJob(C.Structure):  # mm2amd_fin_job_t
    _fields_ = [("query", C.c_void_p), ("target", C.c_void_p), ("qlen", C.c_int32), ("tlen", C.c_int32), ("n_pieces", C.c_int32),
                ("piece", C.POINTER(C.POINTER(C.c_uint32))), ("piece_len", C.POINTER(C.c_int32))]


class FinRes(C.Structure):  # mm2amd_fin_res_t
    _fields_ = [("n_cigar", C.c_int32), ("blen", C.c_int32), ("mlen", C.c_int32), ("n_ambi", C.c_int32), ("dp_max", C.c_int32), ("qshift", C.c_int32),
                ("tshift", C.c_int32), ("is_spliced", C.c_int32), ("cigar_off", C.c_uint32)]


class TxtJob(C.Structure):  # mm2amd_txt_job_t
    _fields_ = [("query", C.c_void_p), ("target", C.c_void_p), ("qlen", C.c_int32), ("tlen", C.c_int32), ("cigar", C.POINTER(C.c_uint32)),
                ("n_cigar", C.c_int32)]


class TxtRes(C.Structure):  # mm2amd_txt_res_t
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("status", C.c_int32)]


class LlJob(C.Structure):  # mm2amd_ll_job_t
    _fields_ = [("query", C.c_void_p), ("target", C.c_void_p), ("qlen", C.c_int32), ("tlen", C.c_int32), ("flag", C.c_int32)]


class LlRes(C.Structure):  # mm2amd_ll_res_t
    _fields_ = [("score", C.c_int32), ("qe", C.c_int32), ("te", C.c_int32), ("path", C.c_int32)]


class SdustJob(C.Structure):  # mm2amd_sdust_job_t
    _fields_ = [("seq", C.c_char_p), ("len", C.c_int32)]


class SdustRes(C.Structure):  # mm2amd_sdust_res_t
    _fields_ = [("off", C.c_uint64), ("n", C.c_uint32), ("path", C.c_int32)]


class HmHit(C.Structure):  # mm2amd_hm_hit_t
    _fields_ = [(n, C.c_int32) for n in ("cnt", "rid", "score", "qs", "qe", "rs", "re", "dp_max")] + [("hash", C.c_uint32), ("flags", C.c_uint32)]


class HmOut(C.Structure):  # mm2amd_hm_out_t
    _fields_ = [(n, C.c_int32) for n in ("pos", "id", "parent", "subsc", "n_sub", "dp_max2")] + [("flags", C.c_uint32), ("reserved", C.c_int32)]


class HmSeg(C.Structure):  # mm2amd_hm_seg_t
    _fields_ = [("n_kept", C.c_int32), ("path", C.c_int32)]


class HmOpt(C.Structure):  # mm2amd_hm_opt_t
    _fields_ = [("mask_level", C.c_float), ("mask_len", C.c_int32), ("pri_ratio", C.c_float), ("best_n", C.c_int32), ("alt_drop", C.c_float),
                ("sub_diff", C.c_int32), ("min_diff", C.c_int32), ("min_strand_sc", C.c_int32), ("flags", C.c_uint32)]


class PeOpt(C.Structure):  # mm2amd_pe_opt_t
    _fields_ = [(n, C.c_int32) for n in ("pe_bonus", "sub_diff", "match_sc", "reserved")]


class FastxRec(C.Structure):  # mm2amd_fastx_rec_t
    _fields_ = [("name", C.c_uint64), ("comment", C.c_uint64), ("seq", C.c_uint64), ("qual", C.c_uint64), ("name_len", C.c_uint32),
                ("comment_len", C.c_uint32), ("l_seq", C.c_int32), ("reserved", C.c_int32)]


class KswRes(C.Structure):  # mm2amd_ksw_res_t
    _fields_ = [(n, C.c_int32) for n in ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score",
                                         "n_cigar", "reach_end")] + [("cigar_off", C.c_uint32)]


class IdxOpt(C.Structure):  # mm_idxopt_t, minimap.h:130-134
    _fields_ = [("k", C.c_short), ("w", C.c_short), ("flag", C.c_short), ("bucket_bits", C.c_short),
                ("mini_batch_size", C.c_int64), ("batch_size", C.c_uint64)]


class MapOpt(C.Structure):  # mm_mapopt_t, minimap.h:136-192
    _fields_ = [("flag", C.c_int64), ("seed", C.c_int), ("sdust_thres", C.c_int), ("max_qlen", C.c_int), ("bw", C.c_int),
                ("bw_long", C.c_int), ("max_gap", C.c_int), ("max_gap_ref", C.c_int), ("max_frag_len", C.c_int),
                ("max_chain_skip", C.c_int), ("max_chain_iter", C.c_int), ("min_cnt", C.c_int), ("min_chain_score", C.c_int),
                ("chain_gap_scale", C.c_float), ("chain_skip_scale", C.c_float), ("rmq_size_cap", C.c_int),
                ("rmq_inner_dist", C.c_int), ("rmq_rescue_size", C.c_int), ("rmq_rescue_ratio", C.c_float),
                ("mask_level", C.c_float), ("mask_len", C.c_int), ("pri_ratio", C.c_float), ("best_n", C.c_int),
                ("alt_drop", C.c_float), ("a", C.c_int), ("b", C.c_int), ("q", C.c_int), ("e", C.c_int), ("q2", C.c_int),
                ("e2", C.c_int), ("transition", C.c_int), ("sc_ambi", C.c_int), ("noncan", C.c_int), ("junc_bonus", C.c_int),
                ("junc_pen", C.c_int), ("zdrop", C.c_int), ("zdrop_inv", C.c_int), ("end_bonus", C.c_int),
                ("min_dp_max", C.c_int), ("min_ksw_len", C.c_int), ("anchor_ext_len", C.c_int), ("anchor_ext_shift", C.c_int),
                ("max_clip_ratio", C.c_float), ("rank_min_len", C.c_int), ("rank_frac", C.c_float), ("pe_ori", C.c_int),
                ("pe_bonus", C.c_int), ("jump_min_match", C.c_int32), ("mid_occ_frac", C.c_float), ("q_occ_frac", C.c_float),
                ("min_mid_occ", C.c_int32), ("max_mid_occ", C.c_int32), ("mid_occ", C.c_int32), ("max_occ", C.c_int32),
                ("max_max_occ", C.c_int32), ("occ_dist", C.c_int32), ("mini_batch_size", C.c_int64), ("max_sw_mat", C.c_int64),
                ("cap_kalloc", C.c_int64), ("split_prefix", C.c_char_p)]


class Extra(C.Structure):  # mm_extra_t header, minimap.h:103-110 (cigar[] follows)
    _fields_ = [("capacity", C.c_uint32), ("dp_score", C.c_int32), ("dp_max", C.c_int32), ("dp_max2", C.c_int32),
                ("dp_max0", C.c_int32), ("n_ambi_strand", C.c_uint32), ("n_cigar", C.c_uint32)]


class Reg1(C.Structure):  # mm_reg1_t, minimap.h:112-127
    _fields_ = [("id", C.c_int32), ("cnt", C.c_int32), ("rid", C.c_int32), ("score", C.c_int32), ("qs", C.c_int32),
                ("qe", C.c_int32), ("rs", C.c_int32), ("re", C.c_int32), ("parent", C.c_int32), ("subsc", C.c_int32),
                ("as_", C.c_int32), ("mlen", C.c_int32), ("blen", C.c_int32), ("n_sub", C.c_int32), ("score0", C.c_int32),
                ("bits", C.c_uint32), ("hash", C.c_uint32), ("div", C.c_float), ("p", C.POINTER(Extra))]

    mapq = property(lambda s: s.bits & 0xff)
    split = property(lambda s: s.bits >> 8 & 3)
    rev = property(lambda s: s.bits >> 10 & 1)
    inv = property(lambda s: s.bits >> 11 & 1)
    sam_pri = property(lambda s: s.bits >> 12 & 1)


class Bseq1(C.Structure):  # mm_bseq1_t, bseq.h:14-17
    _fields_ = [("l_seq", C.c_int), ("rid", C.c_int), ("name", C.c_char_p), ("seq", C.c_char_p), ("qual", C.c_char_p),
                ("comment", C.c_char_p)]


class KernelStat(C.Structure):  # mm2amd_kernel_stat_t
    _fields_ = [("name", C.c_char * 48), ("ms", C.c_double), ("alg_bytes", C.c_double), ("launches", C.c_int64), ("units", C.c_double)]


assert C.sizeof(MapOpt) == 264 and C.sizeof(Reg1) == 80 and C.sizeof(Extra) == 28 and C.sizeof(Bseq1) == 40 and C.sizeof(IdxOpt) == 24

F_CIGAR, F_OUT_SAM = 0x004, 0x008  # MM_F_CIGAR, MM_F_OUT_SAM (minimap.h:12-13)
F_EQX = 0x4000000  # MM_F_EQX (minimap.h:36): --eqx, match operations written as = and X
F_OUT_JUNC = 0x10000000000  # MM_F_OUT_JUNC (minimap.h:50): --write-junc, the splice junctions of the hits instead of SAM / PAF records
I_HPC, I_NO_SEQ, I_NO_NAME = 1, 2, 4  # MM_I_* (minimap.h:41-43)
EINVAL, ENODEV, EHIP, ENOMEM, ESTATE, EIO = -1, -2, -3, -4, -5, -6  # MM2AMD_E*
DUMP_NO_SEQ = 1  # MM2AMD_DUMP_NO_SEQ
TXT_CIGAR, TXT_CS, TXT_CS_LONG, TXT_MD, TXT_DS, TXT_DS_LONG = 0, 1, 2, 3, 4, 5  # MM2AMD_TXT_*
FMT_PATH_DEVICE, FMT_PATH_HOST = 0, 1  # MM2AMD_FMT_PATH_*: who wrote the text of mm_gpu_format_batch_dev
LL_QREV, LL_QCOMP, LL_TREV = 1, 2, 4  # MM2AMD_LL_*
LL_PATH_WAVE, LL_PATH_WG, LL_PATH_HOST = 0, 1, 2  # MM2AMD_LL_PATH_*
SDUST_PATH_NARROW, SDUST_PATH_WIDE = 0, 1  # MM2AMD_SDUST_PATH_*
HM_PATH_NARROW, HM_PATH_WIDE, HM_PATH_HOST = 0, 1, 2  # MM2AMD_HM_PATH_*
HM_REV, HM_INV, HM_ALT, HM_ALIGNED, HM_SAM_PRI, HM_STRAND_RETAINED = 1, 2, 4, 8, 16, 32  # MM2AMD_HM_*: flags of a hit (the last two also of a result)
HM_HARD_MLEVEL, HM_ALL_CHAINS, HM_CHECK_STRAND, HM_WAVE_PARENTS = 1, 2, 4, 8  # MM2AMD_HM_*: flags of the options
PE_PATH_NARROW, PE_PATH_WIDE, PE_PATH_HOST = 0, 1, 2  # MM2AMD_PE_PATH_*
PE_OK, PE_BAD_PARENT = 0, 1  # MM2AMD_PE_*: status of a fragment
PE_REV, PE_SAM_PRI, PE_PROPER_FRAG, PE_THRU = 1, 2, 4, 8  # MM2AMD_PE_*: flags of a hit (the first two) and of a result (the last three)
FASTX_WITH_QUAL, FASTX_WITH_COMMENT = 1, 2  # MM2AMD_FASTX_WITH_*
FASTX_PATH_HOST, FASTX_PATH_FASTQ4, FASTX_PATH_FASTA = 0, 1, 2  # MM2AMD_FASTX_PATH_*
F_COPY_COMMENT, F_FRAG_MODE = 0x2000000, 0x2000  # MM_F_COPY_COMMENT, MM_F_FRAG_MODE (minimap.h:35, :23)

_lib = None


def _bind(L):
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.mm2amd_last_error.restype = C.c_char_p
    L.mm2amd_backend_name.restype = C.c_char_p
    L.mm_gpu_init.argtypes = [vp, vp, C.c_int]
    L.mm_gpu_map_batch.argtypes = [C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, ip]
    L.mm_gpu_batch_stage.argtypes = [C.c_int, ip, ip, vp]
    L.mm_gpu_map_staged.argtypes = [ip, C.POINTER(vp), ip, ip]
    L.mm_gpu_batch_stage_queued.argtypes = [C.c_int, ip, ip, vp]
    L.mm_gpu_batch_discard.restype = None
    L.mm2amd_free_regs.argtypes = [C.c_int, ip, C.POINTER(vp)]
    L.mm2amd_free_regs.restype = None
    L.mm2amd_last_stats.argtypes = [C.POINTER(C.c_double), C.c_int]
    L.mm2amd_pack_regs.argtypes = [C.c_int, ip, C.POINTER(vp), vp, C.c_int64]
    L.mm2amd_pack_regs.restype = C.c_int64
    L.mm2amd_unpack_regs.argtypes = [vp, C.c_int64, C.c_int, ip, C.POINTER(vp)]
    L.mm_gpu_init_multi.argtypes = [vp, vp, C.c_int, C.c_int, ip]
    L.mm_gpu_context_generation.restype = C.c_uint64
    L.mm_gpu_destroy_if.argtypes = [C.c_uint64]
    if hasattr(L, "mm2amd_idx_str"):  # the product library (the CPU check library used by tests has no device index)
        L.mm2amd_ksw_extd2_batch.restype = C.c_int
        L.mm2amd_ksw_extd2_batch.argtypes = [C.c_int, C.POINTER(KswJob), C.c_int8, C.c_char_p, C.c_int8, C.c_int8, C.c_int8,
                                             C.c_int8, C.POINTER(KswRes), C.POINTER(C.c_uint32), C.c_size_t]
        L.mm2amd_ksw_extz2_batch.restype = C.c_int
        L.mm2amd_ksw_extz2_batch.argtypes = [C.c_int, C.POINTER(KswJob), C.c_int8, C.c_char_p, C.c_int8, C.c_int8, C.POINTER(KswRes),
                                             C.POINTER(C.c_uint32), C.c_size_t]
        L.mm2amd_ksw_exts2_batch.restype = C.c_int
        L.mm2amd_ksw_exts2_batch.argtypes = [C.c_int, C.POINTER(KswJob), C.c_int8, C.c_char_p, C.c_int8, C.c_int8, C.c_int8, C.c_int8,
                                             C.POINTER(KswRes), C.POINTER(C.c_uint32), C.c_size_t]
        L.mm2amd_update_extra_batch.restype = C.c_int
        L.mm2amd_update_extra_batch.argtypes = [C.c_int, C.POINTER(FinJob), C.c_char_p, C.c_int8, C.c_int8, C.c_int, C.POINTER(FinRes), C.POINTER(C.c_uint32), C.c_size_t]
        L.mm2amd_update_extra_eqx_batch.restype = C.c_int
        L.mm2amd_update_extra_eqx_batch.argtypes = L.mm2amd_update_extra_batch.argtypes
        L.mm2amd_aln_text_batch.argtypes = [C.c_int, C.POINTER(TxtJob), C.c_int, C.POINTER(TxtRes), vp, C.c_size_t]
        L.mm2amd_hits_text_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(TxtRes), vp,
                                             C.c_size_t]
        L.mm2amd_hits_junc_batch.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_char_p), C.POINTER(TxtRes), vp, C.c_size_t]
        L.mm2amd_idx_getseq.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
        if hasattr(L, "mm2amd_ksw_ll_batch"):
            L.mm2amd_ksw_ll_batch.argtypes = [C.c_int, C.POINTER(LlJob), C.c_int8, C.c_char_p, C.c_int, C.c_int, C.POINTER(LlRes)]
            L.mm2amd_ksw_ll_limits.argtypes = [ip, ip, C.POINTER(C.c_int64), ip]
        if hasattr(L, "mm2amd_sdust_batch"):
            L.mm2amd_sdust_batch.argtypes = [C.c_int, C.POINTER(SdustJob), C.c_int, C.POINTER(SdustRes), vp, C.c_size_t]
            L.mm2amd_sdust_limits.argtypes = [ip, ip, ip]
            L.mm2amd_sdust_host_batch.argtypes = [C.c_int, C.POINTER(SdustJob), C.c_int, C.c_int, C.POINTER(SdustRes), vp, C.c_size_t, C.POINTER(C.c_double)]
        if hasattr(L, "mm2amd_hits_merge_batch"):
            L.mm2amd_hits_merge_batch.argtypes = [C.c_int, vp, vp, C.POINTER(HmOpt), vp, vp]
            L.mm2amd_hits_merge_host_batch.argtypes = [C.c_int, vp, vp, C.POINTER(HmOpt), C.c_int, vp, vp, C.POINTER(C.c_double)]
            L.mm2amd_hits_merge_limits.argtypes = [ip, ip, ip]
        if hasattr(L, "mm2amd_pair_batch"):
            L.mm2amd_pair_batch.argtypes = [C.c_int, vp, vp, C.POINTER(PeOpt), vp, vp]
            L.mm2amd_pair_host_batch.argtypes = [C.c_int, vp, vp, C.POINTER(PeOpt), C.c_int, vp, vp, C.POINTER(C.c_double)]
            L.mm2amd_pair_limits.argtypes = [ip, ip, ip]
        if hasattr(L, "mm2amd_split_open"):
            L.mm2amd_split_open.restype = vp
            L.mm2amd_split_open.argtypes = [C.c_char_p, vp, C.c_int]
            L.mm2amd_split_write.argtypes = [vp, vp, C.c_int, ip, C.POINTER(vp), ip, ip]
            L.mm2amd_split_close.argtypes = [vp]
            L.mm2amd_split_merge_open.restype = vp
            L.mm2amd_split_merge_open.argtypes = [C.c_char_p, C.c_int, vp]
            L.mm2amd_split_merge_batch.argtypes = [vp, C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, ip]
            L.mm2amd_split_merge_format.argtypes = [vp, C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, C.POINTER(vp), C.POINTER(C.c_size_t)]
            L.mm2amd_split_merge_sq.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
            L.mm2amd_split_merge_close.argtypes = [vp, C.c_int]
        if hasattr(L, "mm2amd_fastx_parse"):
            szp = C.POINTER(C.c_size_t)
            L.mm2amd_fastx_parse.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, szp, szp, szp, ip]
            L.mm2amd_fastx_parse_host.argtypes = L.mm2amd_fastx_parse.argtypes
            L.mm2amd_fastx_limits.argtypes = [szp, ip]
            L.mm2amd_fastx_last_times.argtypes = [C.POINTER(C.c_double), C.c_int]
        L.mm2amd_sort_pairs_u64.argtypes = [vp, vp, C.c_uint64, C.c_int]
        L.mm2amd_exclusive_sum_u32.argtypes = [vp, vp, C.c_uint64]
        L.mm2amd_encode_batch.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
        L.mm2amd_encode_range.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, vp]
        L.mm2amd_idx_str.restype = vp
        L.mm2amd_idx_str.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        L.mm2amd_idx_destroy.argtypes = [vp]
        L.mm2amd_idx_destroy.restype = None
        L.mm2amd_idx_stat.argtypes = [vp, ip, ip, ip, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
        L.mm2amd_idx_cal_max_occ.argtypes = [vp, C.c_float]
        L.mm2amd_idx_cal_max_occ.restype = C.c_int32
        L.mm2amd_mapopt_update.argtypes = [vp, vp]
        L.mm2amd_idx_table_shape.argtypes = [vp, ip, ip]
        L.mm2amd_idx_export.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mm2amd_idx_dump.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
        L.mm2amd_idx_load.restype = vp
        L.mm2amd_idx_load.argtypes = [C.c_char_p, C.c_int, ip]
        L.mm2amd_idx_is_idx.argtypes = [C.c_char_p]
        L.mm2amd_idx_seq.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32)]
        L.mm2amd_idx_io_stats.argtypes = [C.POINTER(C.c_double), C.c_int]
        L.mm_gpu_init_index.argtypes = [vp, vp, C.c_int]
        L.mm_gpu_init_index_multi.argtypes = [vp, vp, C.c_int, C.c_int, ip]
        L.mm2amd_set_opt.argtypes = [C.c_char_p, vp, vp]
        L.mm2amd_check_opt.argtypes = [vp, vp]
        L.mm2amd_idxopt_init.argtypes = [vp]
        L.mm2amd_mapopt_init.argtypes = [vp]
        L.mm_gpu_format_batch.argtypes = [C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mm_gpu_format_batch_view.argtypes = [C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.mm_gpu_format_batch_dev.argtypes = [C.c_int, ip, ip, vp, ip, C.POINTER(vp), ip, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), ip]
        L.mm2amd_profile_enable.argtypes = [C.c_int]
        L.mm2amd_profile_enable.restype = None
        L.mm2amd_profile_get.argtypes = [C.POINTER(KernelStat), C.c_int]
    return L


def host_cpus():
    """CPUs this process may use: hardware threads capped by the container's CPU quota"""
    return int(lib().mm2amd_host_cpus())


def _libc_free(p):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(p)


def lib(path=None):
    """Load libmm2amd.so (built in-tree by minimap2_amd.build); raises if it is missing."""
    global _lib
    if path is not None:
        return _bind(C.CDLL(path))
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Mm2AmdError("libmm2amd.so is not built (run `python -m minimap2_amd.build`); there is no CPU fallback")
        _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def _check(rc, L=None):
    if rc != 0:
        e = Mm2AmdError("mm2amd error %d: %s" % (rc, (L or lib()).mm2amd_last_error().decode()))
        e.code = rc
        raise e


# ---------------------------------------------------------------------------------------------------------
# index files (.mmi) and sequence files
# ---------------------------------------------------------------------------------------------------------
def idx_is_idx(fn):
    """mm_idx_is_idx: True when fn is a minimap2 index file, False when it is something else; raises when it cannot be opened"""
    rc = lib().mm2amd_idx_is_idx(os.fsencode(fn))
    if rc < 0:
        _check(rc)
    return rc == 1


def idx_load(fn, part=0):
    """mm2amd_idx_load: (index handle, more) for part `part` of a .mmi file; release the handle with idx_destroy()"""
    L = lib()
    more = C.c_int(0)
    h = L.mm2amd_idx_load(os.fsencode(fn), part, C.byref(more))
    if not h:
        e = Mm2AmdError("mm2amd error %d: %s" % (L.mm2amd_last_error_code(), L.mm2amd_last_error().decode()))
        e.code = L.mm2amd_last_error_code()
        raise e
    return h, bool(more.value)


def idx_dump(idx, fn, bucket_bits=0, flags=0):
    """mm2amd_idx_dump: the index behind the handle as one part of a .mmi file"""
    _check(lib().mm2amd_idx_dump(idx, os.fsencode(fn), bucket_bits, flags))


def idx_destroy(idx):
    lib().mm2amd_idx_destroy(idx)


def idx_io_stats():
    """phases of the last idx_dump / idx_load of this process (milliseconds, bytes)"""
    v = (C.c_double * 16)()
    n = lib().mm2amd_idx_io_stats(v, 16)
    names = ["total_ms", "regroup_ms", "kernel_ms", "copy_ms", "file_ms", "sort_ms", "tables_ms", "seq_ms", "image_bytes", "file_bytes", "n_chunks", "chunk_bytes"]
    return dict(zip(names, list(v)[:n]))


def read_fastx(fn):
    """The records of a FASTA / FASTQ file, plain or gzip, as (names, sequences) -- lists of bytes; a name ends at the first blank, as kseq's does."""
    import gzip
    with open(fn, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    names, seqs = [], []
    with (gzip.open(fn, "rb") if gz else open(fn, "rb")) as f:
        data = f.read()
    lines = data.split(b"\n")
    i, n = 0, len(lines)
    while i < n:
        ln = lines[i].rstrip(b"\r")
        i += 1
        if not ln:
            continue
        if ln[:1] == b">":
            names.append(ln[1:].split(None, 1)[0] if len(ln) > 1 and ln[1:].split() else b"")
            parts = []
            while i < n and lines[i][:1] not in (b">", b"@"):
                parts.append(lines[i].strip())
                i += 1
            seqs.append(b"".join(parts))
        elif ln[:1] == b"@":
            names.append(ln[1:].split(None, 1)[0] if len(ln) > 1 and ln[1:].split() else b"")
            parts, got = [], 0
            while i < n and lines[i][:1] != b"+":
                parts.append(lines[i].strip())
                i += 1
            seqs.append(b"".join(parts))
            i += 1  # the '+' line
            while i < n and got < len(seqs[-1]):  # as many quality characters as there are bases
                got += len(lines[i].strip())
                i += 1
        else:
            raise Mm2AmdError("%s: neither FASTA nor FASTQ (line %d)" % (fn, i))
    if not seqs:
        raise Mm2AmdError("%s: no sequence" % fn)
    return names, seqs


def _fastx_call(data, is_final, flags, device, L=None):
    """mm2amd_fastx_parse (device) / mm2amd_fastx_parse_host over a bytes-like `data`: (table, pool, consumed, path) -- the table a numpy
    record array with the fields of mm2amd_fastx_rec_t, entries with reserved != 0 included, the pool a numpy uint8 array"""
    import numpy as np
    L = L or lib()
    text = np.frombuffer(data, dtype=np.uint8)
    call = L.mm2amd_fastx_parse if device else L.mm2amd_fastx_parse_host
    n, pl, used, path = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    rec_cap, pool_cap = text.size // 64 + 16, text.size + 16  # a guess that holds for reads of 30 bases and more; the sizes come back otherwise
    while True:
        recs, pool = np.empty(rec_cap, dtype=_fastx_dtype()), np.empty(pool_cap, dtype=np.uint8)
        rc = call(text.ctypes.data if text.size else None, text.size, 1 if is_final else 0, flags, recs.ctypes.data, rec_cap, pool.ctypes.data, pool_cap,
                  C.byref(n), C.byref(pl), C.byref(used), C.byref(path))
        if rc == ENOMEM and (n.value > rec_cap or pl.value > pool_cap):
            rec_cap, pool_cap = max(rec_cap, n.value), max(pool_cap, pl.value)
            continue
        _check(rc, L)
        return recs[:n.value], pool[:pl.value], used.value, path.value


def _fastx_dtype():
    import numpy as np
    return np.dtype([("name", "<u8"), ("comment", "<u8"), ("seq", "<u8"), ("qual", "<u8"), ("name_len", "<u4"), ("comment_len", "<u4"), ("l_seq", "<i4"),
                     ("reserved", "<i4")])


def parse_fastx(data, is_final=True, with_qual=True, with_comment=False, device=True):
    """The complete records of a block of FASTA / FASTQ text, as kseq_read + kseq2bseq return them (mm2amd_fastx_parse; device=False: the host's
    parser, mm2amd_fastx_parse_host).  Returns (records, consumed, path): each record (name, comment | None, seq, qual | None) as bytes;
    consumed, the offset of the first byte that belongs to no complete record (put data[consumed:] in front of the next block); path, who
    parsed it (FASTX_PATH_FASTQ4 / FASTX_PATH_FASTA: the kernels; FASTX_PATH_HOST: the host).  Malformed records are left out."""
    flags = (FASTX_WITH_QUAL if with_qual else 0) | (FASTX_WITH_COMMENT if with_comment else 0)
    recs, pool, used, path = _fastx_call(data, is_final, flags, device)
    raw, none, out = pool.tobytes(), 0xffffffffffffffff, []
    for r in recs.tolist():
        if r[7]:
            continue
        out.append((raw[r[0]:r[0] + r[4]], None if r[1] == none else raw[r[1]:r[1] + r[5]], raw[r[2]:r[2] + r[6]],
                    None if r[3] == none else raw[r[3]:r[3] + r[6]]))
    return out, used, path


def fastx_limits():
    """mm2amd_fastx_limits: max_text, the longest block the device path takes, and long_line as in force"""
    a, b = C.c_size_t(0), C.c_int(0)
    _check(lib().mm2amd_fastx_limits(C.byref(a), C.byref(b)))
    return {"max_text": a.value, "long_line": b.value}


def _qname_len(s):  # mm_qname_len (bseq.h:31-36)
    n = len(s)
    return n - 2 if n >= 3 and 48 <= s[n - 1] <= 57 and s[n - 2] == 47 else n


def _qname_same(a, b):  # mm_qname_same (bseq.h:38-44)
    la, lb = _qname_len(a), _qname_len(b)
    return la == lb and a[:la] == b[:lb]


class _FastxSource(object):
    """One sequence file as a stream of parsed blocks: text is read block_bytes at a time behind the unconsumed tail of the block before; a
    block without a complete record is read again with twice the room."""

    def __init__(self, fn, flags, block_bytes, device):
        import gzip
        with open(fn, "rb") as f:
            gz = f.read(2) == b"\x1f\x8b"
        self.f = gzip.open(fn, "rb") if gz else open(fn, "rb")  # (decompression stays on the host: the library links no zlib)
        self.flags, self.block, self.device = flags, max(int(block_bytes), 16), device
        self.tail, self.done = b"", False
        self.recs, self.pool, self.i = None, None, 0
        self.paths = []  # who parsed each block (FASTX_PATH_*)

    def close(self):
        self.f.close()

    def fill(self):
        """make self.recs[self.i] the next table entry; False at the end of the file"""
        while self.recs is None or self.i >= len(self.recs):
            if self.done:
                return False
            want = self.block
            while True:
                data = self.f.read(want)
                final = len(data) < want
                text = memoryview(self.tail + data if self.tail else data)
                if self.device and len(text) > fastx_limits()["max_text"]:
                    raise Mm2AmdError("a single record outgrows the longest block the device reader takes; read the file with device=False")
                recs, pool, used, path = _fastx_call(text, final, self.flags, self.device)
                self.paths.append(path)
                if final or len(recs):
                    break
                self.tail, want = bytes(text), max(want, len(text))  # no complete record: the same text and as much again
            self.tail = b"" if final else bytes(text[used:])
            self.done = final
            self.recs, self.pool, self.i = recs, pool, 0
            self.bad = recs["reserved"] != 0
            self.l_seq = recs["l_seq"].astype("int64")
        return True

    def name(self, i):
        r = self.recs[i]
        return self.pool[int(r["name"]):int(r["name"]) + int(r["name_len"])].tobytes()

    def run(self):
        """how many entries from self.i on are good ones"""
        import numpy as np
        b = np.flatnonzero(self.bad[self.i:])
        return int(b[0]) if len(b) else len(self.recs) - self.i


class FastxReader(object):
    """The batches mm_bseq_read3 (bseq.c:80-119) -- or, for a list of two or more files, mm_bseq_read_frag2 (bseq.c:131-159) -- returns for
    successive calls with chunk_size = chunk_bases, as Batch objects with the fragment table of map.c:560-575; iteration ends, like the
    reference's pipeline, with the first call that returns no record.  Plain or gzip files.  The records come from mm2amd_fastx_parse (device=True:
    fastx_lines_kernel / fastx_classify_kernel / fastx_copy_kernel, the host's parser for text that is neither plain FASTA nor four-line FASTQ)
    or from the host's parser alone (device=False); the batches are the same.
    with_qual / with_comment: keep the qualities / the comments (kseq2bseq).  frag_mode: MM_F_FRAG_MODE -- a pair is not split across batches and
    reads of one name form a fragment.  The text is read block_bytes at a time.  paths lists who parsed each block."""

    def __init__(self, fn_or_list, chunk_bases=500_000_000, with_qual=True, with_comment=False, frag_mode=False, block_bytes=64 << 20, device=True):
        fns = [fn_or_list] if isinstance(fn_or_list, (str, bytes, os.PathLike)) else list(fn_or_list)
        if not fns:
            raise Mm2AmdError("FastxReader needs a file")
        flags = (FASTX_WITH_QUAL if with_qual else 0) | (FASTX_WITH_COMMENT if with_comment else 0)
        self.src = [_FastxSource(fn, flags, block_bytes, device) for fn in fns]
        self.chunk_bases, self.frag_mode = int(chunk_bases), bool(frag_mode) or len(fns) > 1
        self.n_processed = 0
        self._stash = None  # (source chunk, index) of the read mm_bseq_read3 keeps for its next call

    @property
    def paths(self):
        return [p for s in self.src for p in s.paths]

    def close(self):
        for s in self.src:
            s.close()

    def __iter__(self):
        try:
            while True:
                parts = self._read_frag2() if len(self.src) > 1 else self._read3()
                if not parts:
                    return
                yield self._batch(parts)
        finally:
            self.close()

    # a part: (recs, pool, lo, hi) -- entries lo .. hi - 1 of one parsed block
    def _read3(self):
        import numpy as np
        s, parts, size = self.src[0], [], 0
        if self._stash is not None:
            parts.append(self._stash)
            size = int(self._stash[0][self._stash[2]]["l_seq"])
            self._stash = None
        while s.fill():
            n_good = s.run()
            if n_good == 0:  # a malformed record: mm_bseq_read3 returns what it has
                s.i += 1
                return parts
            cum = np.cumsum(s.l_seq[s.i:s.i + n_good]) + size
            k = int(np.searchsorted(cum, self.chunk_bases, side="left"))  # the first record with which the batch holds chunk_bases bases
            if k >= n_good:
                parts.append((s.recs, s.pool, s.i, s.i + n_good))
                size, s.i = int(cum[-1]), s.i + n_good
                continue
            parts.append((s.recs, s.pool, s.i, s.i + k + 1))
            s.i += k + 1
            if self.frag_mode and int(parts[-1][0][parts[-1][3] - 1]["l_seq"]) < 1000000:  # the rest of the pair (bseq.c:100-109)
                last = self._name(parts[-1])
                while s.fill():
                    if s.bad[s.i]:
                        s.i += 1
                        break
                    one = (s.recs, s.pool, s.i, s.i + 1)
                    s.i += 1
                    if not _qname_same(self._name(one), last):
                        self._stash = one
                        break
                    parts.append(one)
                    last = self._name(one)
            return parts
        return parts

    @staticmethod
    def _name(part):
        r = part[0][part[3] - 1]
        return part[1][int(r["name"]):int(r["name"]) + int(r["name_len"])].tobytes()

    def _read_frag2(self):
        import numpy as np
        parts, size = [], 0  # a part here: a tuple of one part per file, interleaved record by record
        while True:
            have = [s.fill() for s in self.src]
            k = min(s.run() if h else 0 for s, h in zip(self.src, have))
            if k == 0:  # a file has ended or holds a malformed record: the round's other records are dropped (bseq.c:140-147)
                for s, h in zip(self.src, have):
                    if h:
                        s.i += 1
                return parts
            per_round = sum(s.l_seq[s.i:s.i + k] for s in self.src)
            cum = np.cumsum(per_round) + size
            j = int(np.searchsorted(cum, self.chunk_bases, side="left"))
            take = k if j >= k else j + 1
            parts.append(tuple((s.recs, s.pool, s.i, s.i + take) for s in self.src))
            for s in self.src:
                s.i += take
            size = int(cum[take - 1])
            if j < k:
                return parts

    def _batch(self, parts):
        import numpy as np
        dt = np.dtype([("l_seq", "<i4"), ("rid", "<i4"), ("name", "<u8"), ("seq", "<u8"), ("qual", "<u8"), ("comment", "<u8")])
        none = np.uint64(0xffffffffffffffff)

        def records(part):
            recs, pool, lo, hi = part
            r, base = recs[lo:hi], np.uint64(pool.ctypes.data)
            a = np.zeros(hi - lo, dtype=dt)
            a["l_seq"], a["name"], a["seq"] = r["l_seq"], r["name"] + base, r["seq"] + base
            a["qual"] = np.where(r["qual"] == none, np.uint64(0), r["qual"] + base)
            a["comment"] = np.where(r["comment"] == none, np.uint64(0), r["comment"] + base)
            return a
        chunks, keep = [], []
        for p in parts:
            if isinstance(p[0], tuple):  # one part per file: record k of every file, then record k + 1
                cols = [records(q) for q in p]
                a = np.empty((len(cols[0]), len(cols)), dtype=dt)
                for c, col in enumerate(cols):
                    a[:, c] = col
                chunks.append(a.reshape(-1))
                keep.extend(q[1] for q in p)
            else:
                chunks.append(records(p))
                keep.append(p[1])
        arr = np.concatenate(chunks) if len(chunks) > 1 else chunks[0]
        n = len(arr)
        arr["rid"] = np.arange(self.n_processed, self.n_processed + n, dtype=np.int64).astype(np.int32)  # (map.c:555-556)
        self.n_processed += n
        if self.frag_mode:  # reads of one name, next to each other, are one fragment (map.c:566-571)
            names = [C.string_at(int(a)) for a in arr["name"]]
            starts = [0] + [i for i in range(1, n) if not _qname_same(names[i - 1], names[i])]
            seg_off = np.array(starts, dtype=np.int32)
        else:
            seg_off = np.arange(n, dtype=np.int32)
        n_seg = np.diff(np.append(seg_off, np.int32(n))).astype(np.int32)
        return Batch.from_pool(arr, keep, seg_off, n_seg)


def fin_jobs(jobs):
    """jobs of update_extra_batch as the C ABI's array: (FinJob array, the objects it points into -- keep them alive --, the sum of the piece lengths)"""
    n = len(jobs)
    arr = (FinJob * max(n, 1))()
    keep, tot = [], 0
    for i, (qs, ts, pieces) in enumerate(jobs):
        qb, tb = bytes(qs), bytes(ts)
        parr = [(C.c_uint32 * max(len(p_), 1))(*p_) for p_ in pieces]
        pp = (C.POINTER(C.c_uint32) * max(len(pieces), 1))(*[C.cast(a, C.POINTER(C.c_uint32)) for a in parr])
        pl = (C.c_int32 * max(len(pieces), 1))(*[len(p_) for p_ in pieces])
        keep.append((qb, tb, parr, pp, pl))
        arr[i].query, arr[i].target = C.cast(C.c_char_p(qb), C.c_void_p), C.cast(C.c_char_p(tb), C.c_void_p)
        arr[i].qlen, arr[i].tlen, arr[i].n_pieces, arr[i].piece, arr[i].piece_len = len(qb), len(tb), len(pieces), pp, pl
        tot += sum(len(p_) for p_ in pieces)
    return arr, keep, tot


def update_extra_batch(jobs, mat, q, e, log_gap, eqx=False):
    """jobs: list of (query_codes, target_codes, [piece, ...]) -- nt4 codes 0..4 of the aligned stretches and the windows' CIGARs (sequences of
    len << 4 | op) in alignment order.  Returns a list of (cigar_tuple, blen, mlen, n_ambi, dp_max, qshift, tshift, is_spliced) -- what the
    reference's mm_update_extra (align.c:254-303) leaves in the hit record -- or None for a region whose operations do not cover its stretches.
    eqx: with is_eqx set -- the matches cut into = and X (mm_update_cigar_eqx, align.c:183-252; mm2amd_update_extra_eqx_batch)."""
    n = len(jobs)
    arr, keep, tot = fin_jobs(jobs)
    res = (FinRes * max(n, 1))()
    if eqx:  # the sizing call, then the real one
        _check(lib().mm2amd_update_extra_eqx_batch(n, arr, bytes(mat), q, e, 1 if log_gap else 0, res, None, 0))
        tot = sum(max(r.n_cigar, 0) for r in res[:n])
    pool = (C.c_uint32 * max(tot, 1))()
    call = lib().mm2amd_update_extra_eqx_batch if eqx else lib().mm2amd_update_extra_batch
    _check(call(n, arr, bytes(mat), q, e, 1 if log_gap else 0, res, pool, max(tot, 1)))
    out = []
    for i in range(n):
        r = res[i]
        out.append(None if r.n_cigar < 0 else (tuple(pool[r.cigar_off:r.cigar_off + r.n_cigar]), r.blen, r.mlen, r.n_ambi, r.dp_max, r.qshift, r.tshift, r.is_spliced))
    return out


def _texts(call, n):
    """the sizing call, then the real one: a list of str, None for a job the kernel refused"""
    res = (TxtRes * max(n, 1))()
    _check(call(res, None, 0))
    total = sum(r.len for r in res[:n])
    pool = C.create_string_buffer(max(total, 1))
    _check(call(res, pool, total))
    raw = pool.raw
    return [None if r.status != 0 else raw[r.off:r.off + r.len].decode("ascii") for r in res[:n]]


def aln_text_batch(jobs, what):
    """jobs: list of (query_codes, target_codes, cigar) -- nt4 codes 0..4 of the aligned stretches and the CIGAR as len << 4 | op words; the
    sequences may be None for TXT_CIGAR.  what: TXT_CIGAR, TXT_CS, TXT_CS_LONG, TXT_MD, TXT_DS or TXT_DS_LONG.  Returns each job's text (what the
    reference's mm_gen_cs / mm_gen_ds / mm_gen_MD return, format.c:364-395; aln_text_kernel), or None for a job whose operations the kernel refuses."""
    n = len(jobs)
    arr = (TxtJob * max(n, 1))()
    keep = []
    for i, (q, t, cig) in enumerate(jobs):
        qb, tb = (None if q is None else bytes(q)), (None if t is None else bytes(t))
        ca = (C.c_uint32 * max(len(cig), 1))(*cig)
        keep.append((qb, tb, ca))
        arr[i].query, arr[i].target = C.cast(C.c_char_p(qb), C.c_void_p), C.cast(C.c_char_p(tb), C.c_void_p)
        arr[i].qlen, arr[i].tlen, arr[i].cigar, arr[i].n_cigar = len(qb or b""), len(tb or b""), ca, len(cig)
    L = lib()
    return _texts(lambda res, pool, cap: L.mm2amd_aln_text_batch(n, arr, what, res, pool, cap), n)


def ksw_ll_batch(jobs, mat, gapo, gape):
    """jobs: list of (query_codes, target_codes) or (query_codes, target_codes, flag) -- nt4 codes 0..4; flag: LL_QREV | LL_QCOMP | LL_TREV, how the
    sequences are read.  Returns a list of (score, qe, te, path): what the reference's ksw_ll_qinit + ksw_ll_i16 (ksw2_ll_sse.c:37-152) return on
    the sequences so transformed, and where the job ran (LL_PATH_WAVE / LL_PATH_WG: ksw_ll_kernel; LL_PATH_HOST: the host's scalar routine)."""
    n = len(jobs)
    arr = (LlJob * max(n, 1))()
    keep = []
    for i, j in enumerate(jobs):
        qb, tb = bytes(j[0]), bytes(j[1])
        keep.append((qb, tb))
        arr[i].query, arr[i].target = C.cast(C.c_char_p(qb), C.c_void_p), C.cast(C.c_char_p(tb), C.c_void_p)
        arr[i].qlen, arr[i].tlen, arr[i].flag = len(qb), len(tb), (j[2] if len(j) > 2 else 0)
    res = (LlRes * max(n, 1))()
    _check(lib().mm2amd_ksw_ll_batch(n, arr, 5, bytes(mat), gapo, gape, res))
    return [(r.score, r.qe, r.te, r.path) for r in res[:n]]


def ksw_ll_limits():
    """mm2amd_ksw_ll_limits: the shapes behind ksw_ll_batch's routing -- strip_cols, wg_waves, wg_min_cells (as in force), max_len"""
    a, b, d, c = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    _check(lib().mm2amd_ksw_ll_limits(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return {"strip_cols": a.value, "wg_waves": b.value, "wg_min_cells": c.value, "max_len": d.value}


def _sdust_jobs(seqs):
    n = len(seqs)
    arr = (SdustJob * max(n, 1))()
    keep = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    for i, b in enumerate(keep):
        arr[i].seq, arr[i].len = b, len(b)
    return arr, keep


def _sdust_regions(call, n, keep):
    """per job an (n, 2) int32 array of (start, finish), and the result records.  One call: a region is at least four bases long and two regions
    never touch, so a sequence of len bases has at most len // 4 + 1 of them and the pool can be sized without the sizing call (a second scan)."""
    import numpy as np
    res = (SdustRes * max(n, 1))()
    cap = sum(len(b) // 4 + 1 for b in keep)
    pool = np.zeros(max(cap, 1), dtype=np.uint64)
    _check(call(res, pool.ctypes.data, cap))
    out = []
    for r in res[:n]:
        v = pool[r.off:r.off + r.n]
        out.append(np.stack([(v >> np.uint64(32)).astype(np.int32), (v & np.uint64(0xffffffff)).astype(np.int32)], axis=1).reshape(-1, 2))
    return out, res


def sdust_batch(seqs, T=20, paths=False):
    """mm2amd_sdust_batch: seqs a list of bytes / str (ASCII, as the reference's sdust() takes them).  Returns per sequence an (n, 2) int32
    array of the (start, finish) pairs sdust(seq, T, W = 64) returns (sdust.c:134-175; sdust_kernel, one wavefront per sequence); with
    paths=True also the list of launch classes that scanned them (SDUST_PATH_NARROW / SDUST_PATH_WIDE)."""
    n = len(seqs)
    arr, keep = _sdust_jobs(seqs)
    L = lib()
    out, res = _sdust_regions(lambda res, pool, cap: L.mm2amd_sdust_batch(n, arr, T, res, pool, cap), n, keep)
    return (out, [r.path for r in res[:n]]) if paths else out


def sdust_host_batch(seqs, T=20, n_threads=1):
    """mm2amd_sdust_host_batch: the same regions from the host's sdust_scan on n_threads threads; returns (regions, core_seconds)"""
    n = len(seqs)
    arr, keep = _sdust_jobs(seqs)
    L = lib()
    cs = C.c_double(0)
    out, _ = _sdust_regions(lambda res, pool, cap: L.mm2amd_sdust_host_batch(n, arr, T, n_threads, res, pool, cap, C.byref(cs)), n, keep)
    return out, cs.value


def sdust_limits():
    """mm2amd_sdust_limits: narrow_cap (as in force), wide_cap, max_len -- a sequence takes the wide class iff its list of perfect intervals
    ever held more than narrow_cap entries"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().mm2amd_sdust_limits(C.byref(a), C.byref(b), C.byref(c)))
    return {"narrow_cap": a.value, "wide_cap": b.value, "max_len": c.value}


HM_HIT_DTYPE = [(n, "<i4") for n in ("cnt", "rid", "score", "qs", "qe", "rs", "re", "dp_max")] + [("hash", "<u4"), ("flags", "<u4")]
HM_OUT_DTYPE = [(n, "<i4") for n in ("pos", "id", "parent", "subsc", "n_sub", "dp_max2")] + [("flags", "<u4"), ("reserved", "<i4")]


def hm_opt(mask_level=0.5, mask_len=0x7fffffff, pri_ratio=0.8, best_n=5, alt_drop=0.15, sub_diff=8, min_diff=30, min_strand_sc=4000, flags=0):
    """mm2amd_hm_opt_t; the defaults are minimap2's (a = 2, b = 4: sub_diff = 2 a + b; k = 15: min_diff = 2 k; max_gap = 5000)"""
    return HmOpt(mask_level, mask_len, pri_ratio, best_n, alt_drop, sub_diff, min_diff, min_strand_sc, flags)


def _hm_call(call, segs, opt):
    import numpy as np
    n = len(segs)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(s) for s in segs], dtype=np.uint64)
    hits = np.zeros(max(int(off[n]), 1), dtype=HM_HIT_DTYPE)
    for s, o in zip(segs, off):
        hits[int(o):int(o) + len(s)] = np.asarray(s, dtype=HM_HIT_DTYPE)
    out = np.zeros(max(int(off[n]), 1), dtype=HM_OUT_DTYPE)
    seg = np.zeros((max(n, 1), 2), dtype=np.int32)
    _check(call(n, off.ctypes.data, hits.ctypes.data, C.byref(opt), out.ctypes.data, seg.ctypes.data))
    return [out[int(off[i]):int(off[i + 1])].copy() for i in range(n)], [int(x) for x in seg[:n, 0]], [int(x) for x in seg[:n, 1]]


def hits_merge_batch(segs, opt=None):
    """mm2amd_hits_merge_batch: segs a list of per-segment hit lists, each a structured array of HM_HIT_DTYPE (the records of all index parts in
    part order, rid shifted, dp_max after mm_update_dp_max).  The rules of merge_hits (map.c:520-531) between mm_update_dp_max and mm_set_mapq2 on
    hits_merge_kernel, one wavefront per segment.  Returns (out, n_kept, path): per segment an HM_OUT_DTYPE array answering its hits one by one
    (pos -1: dropped), the length of its final list, and the class that ran it (HM_PATH_*)."""
    L = lib()
    return _hm_call(lambda n, off, hits, o, out, seg: L.mm2amd_hits_merge_batch(n, off, hits, o, out, seg), segs, opt or hm_opt())


def hits_merge_host_batch(segs, opt=None, n_threads=1, wave_parents=False):
    """mm2amd_hits_merge_host_batch: the same rules on n_threads host threads (path is HM_PATH_HOST throughout); wave_parents=True runs the kernel's
    lane-wise form of mm_set_parent.  Returns (out, n_kept, path, core_seconds)."""
    L = lib()
    o = opt or hm_opt()
    if wave_parents:
        o = HmOpt.from_buffer_copy(o)
        o.flags |= HM_WAVE_PARENTS
    cs = C.c_double(0)
    r = _hm_call(lambda n, off, hits, oo, out, seg: L.mm2amd_hits_merge_host_batch(n, off, hits, oo, n_threads, out, seg, C.byref(cs)), segs, o)
    return r + (cs.value,)


def hits_merge_limits():
    """mm2amd_hits_merge_limits: narrow_cap and wide_cap (hits a segment may have in either launch class), max_hits (of a segment at all)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().mm2amd_hits_merge_limits(C.byref(a), C.byref(b), C.byref(c)))
    return {"narrow_cap": a.value, "wide_cap": b.value, "max_hits": c.value}


PE_HIT_DTYPE = [(n, "<i4") for n in ("rid", "rs", "re", "qs", "qe", "dp_max", "id", "parent", "mapq")] + [("hash", "<u4"), ("flags", "<u4"), ("reserved", "<u4")]
PE_OUT_DTYPE = [("parent", "<i4"), ("mapq", "<i4"), ("flags", "<u4"), ("reserved", "<i4")]
PE_FRAG_DTYPE = [("hit0", "<u8"), ("n", "<i4", (2,)), ("qlen", "<i4", (2,)), ("max_gap_ref", "<i4"), ("reserved", "<i4")]  # mm2amd_pe_frag_t
PE_RES_DTYPE = [("path", "<i4"), ("status", "<i4"), ("n_pairs", "<i4"), ("best", "<i4", (2,)), ("reserved", "<i4")]  # mm2amd_pe_res_t


def _pe_call(call, frags, pe_bonus, sub_diff, match_sc):
    import numpy as np
    n = len(frags)
    fr = np.zeros(max(n, 1), dtype=PE_FRAG_DTYPE)
    at = 0
    for i, (h0, h1, qlens, gap) in enumerate(frags):
        fr[i]["hit0"], fr[i]["n"], fr[i]["qlen"], fr[i]["max_gap_ref"] = at, (len(h0), len(h1)), tuple(qlens), gap
        at += len(h0) + len(h1)
    hits = np.zeros(max(at, 1), dtype=PE_HIT_DTYPE)
    for i, (h0, h1, _, _) in enumerate(frags):
        o = int(fr[i]["hit0"])
        hits[o:o + len(h0)] = np.asarray(h0, dtype=PE_HIT_DTYPE)
        hits[o + len(h0):o + len(h0) + len(h1)] = np.asarray(h1, dtype=PE_HIT_DTYPE)
    out = np.zeros(max(at, 1), dtype=PE_OUT_DTYPE)
    res = np.zeros(max(n, 1), dtype=PE_RES_DTYPE)
    opt = PeOpt(pe_bonus, sub_diff, match_sc, 0)
    _check(call(n, fr.ctypes.data, hits.ctypes.data, C.byref(opt), out.ctypes.data, res.ctypes.data))
    outs = []
    for i in range(n):
        o, n0, n1 = int(fr[i]["hit0"]), int(fr[i]["n"][0]), int(fr[i]["n"][1])
        outs.append((out[o:o + n0].copy(), out[o + n0:o + n0 + n1].copy()))
    return outs, res[:n].copy()


def pair_batch(frags, pe_bonus=33, sub_diff=8, match_sc=2):
    """mm2amd_pair_batch: mm_pair and mm_set_pe_thru (pe.c:50-68, :81-182) on pair_kernel, one wavefront per fragment.  frags is a list of
    (hits of segment 0, hits of segment 1, (qlen0, qlen1), max_gap_ref), the hits structured arrays of PE_HIT_DTYPE as they stand after
    mm_set_mapq2; the defaults are minimap2's (a = 2, b = 4: sub_diff = 2 a + b, match_sc = a).  Returns (out, res): per fragment a pair of
    PE_OUT_DTYPE arrays answering its hits one by one, and a PE_RES_DTYPE array (path: PE_PATH_*, status: PE_OK / PE_BAD_PARENT, n_pairs, best)."""
    L = lib()
    return _pe_call(lambda n, fr, hits, o, out, res: L.mm2amd_pair_batch(n, fr, hits, o, out, res), frags, pe_bonus, sub_diff, match_sc)


def pair_host_batch(frags, pe_bonus=33, sub_diff=8, match_sc=2, n_threads=1):
    """mm2amd_pair_host_batch: the same rules on n_threads host threads (path is PE_PATH_HOST throughout).  Returns (out, res, core_seconds)."""
    L = lib()
    cs = C.c_double(0)
    r = _pe_call(lambda n, fr, hits, o, out, res: L.mm2amd_pair_host_batch(n, fr, hits, o, n_threads, out, res, C.byref(cs)), frags, pe_bonus, sub_diff, match_sc)
    return r + (cs.value,)


def pair_limits():
    """mm2amd_pair_limits: narrow_cap and wide_cap (ends -- hits of both segments -- a fragment may have in either launch class), max_hits (of a segment at all)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().mm2amd_pair_limits(C.byref(a), C.byref(b), C.byref(c)))
    return {"narrow_cap": a.value, "wide_cap": b.value, "max_hits": c.value}


def hits_text(idx, hits, reads, what, is_qstrand=False):
    """mm2amd_hits_text_batch: idx an index handle, hits the addresses of mm_reg1_t records, reads each hit's read (bytes).  Returns each
    hit's text, '' for a hit without base-level alignment (mm_gen_cs_ds_or_MD, format.c:364-375)."""
    n = len(hits)
    harr = (C.c_void_p * max(n, 1))(*hits)
    rb = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    qarr, qlen = (C.c_char_p * max(n, 1))(*rb), (C.c_int32 * max(n, 1))(*[len(r) for r in rb])
    L = lib()
    return _texts(lambda res, pool, cap: L.mm2amd_hits_text_batch(idx, n, harr, qarr, qlen, what, 1 if is_qstrand else 0, res, pool, cap), n)


def hits_junc(idx, hits, names):
    """mm2amd_hits_junc_batch: idx an index handle, hits the addresses of mm_reg1_t records, names each hit's read name.  Returns each hit's
    junction lines as mm_write_junc (format.c:263-300) leaves them -- joined by '\\n', none at the end; '' for a hit that writes nothing, None
    for one whose CIGAR the kernel refuses."""
    n = len(hits)
    harr = (C.c_void_p * max(n, 1))(*hits)
    narr = (C.c_char_p * max(n, 1))(*[x.encode() if isinstance(x, str) else bytes(x) for x in names])
    L = lib()
    return _texts(lambda res, pool, cap: L.mm2amd_hits_junc_batch(idx, n, harr, narr, res, pool, cap), n)


def sort_pairs_u64(keys, vals, bits=64):
    """(keys, vals) -- numpy uint64 arrays of equal length -- sorted by key bits [0, bits), stably, on the device (the index build's sort,
    device_sort.hip).  Returns new arrays."""
    import numpy as np
    k, v = np.ascontiguousarray(keys, dtype=np.uint64).copy(), np.ascontiguousarray(vals, dtype=np.uint64).copy()
    assert k.shape == v.shape and k.ndim == 1
    _check(lib().mm2amd_sort_pairs_u64(k.ctypes.data, v.ctypes.data, k.size, bits))
    return k, v


def exclusive_sum_u32(a):
    """numpy uint32 array of n entries -> n + 1 running sums mod 2^32, on the device (device_sort.hip)"""
    import numpy as np
    x = np.ascontiguousarray(a, dtype=np.uint32)
    out = np.empty(x.size + 1, dtype=np.uint32)
    _check(lib().mm2amd_exclusive_sum_u32(x.ctypes.data, out.ctypes.data, x.size))
    return out


def encode_batch(reads, lo=0, hi=None):
    """mm2amd_encode_batch: encode_kernel, with the mapper's launch shape, on a batch of its own.  reads: bytes, or (bytes, bytes) for a pair
    (two units).  lo / hi: launch on reads[lo:hi] only, as a mapper lane does on its sub-batch (mm2amd_encode_range).  Returns (pool, unit_off): pool a numpy uint8 array of 16 guard bytes 0xff | the query pool | 16 guard bytes 0xff (the pool
    is 0xff wherever the kernel did not write), unit_off the units' base offsets (n_units + 1): the unit at o = unit_off[u] has its forward
    codes at pool[16 + 2 * o + j] and its reverse complement at pool[16 + 2 * o + 2 * len - 1 - j]."""
    import numpy as np
    n = len(reads)
    pairs = [r if isinstance(r, tuple) else (r, b"") for r in reads]
    bufs = [bytes(a) + bytes(b) for a, b in pairs]
    unit_off = [0]
    for a, b in pairs:
        unit_off.append(unit_off[-1] + len(a))
        if len(b) > 0:
            unit_off.append(unit_off[-1] + len(b))
    seqs = (C.c_char_p * max(n, 1))(*bufs)
    lens = (C.c_int32 * max(n, 1))(*[len(a) for a, _ in pairs])
    lens2 = (C.c_int32 * max(n, 1))(*[len(b) for _, b in pairs])
    out = np.empty(2 * unit_off[-1] + 32, dtype=np.uint8)
    if lo == 0 and hi is None:
        _check(lib().mm2amd_encode_batch(n, seqs, lens, lens2, out.ctypes.data))
    else:
        _check(lib().mm2amd_encode_range(n, seqs, lens, lens2, lo, n if hi is None else hi, out.ctypes.data))
    return out, np.array(unit_off, dtype=np.int64)


def ksw_extz2_batch(jobs, mat, gapo, gape):
    """single-affine twin of ksw_extd2_batch (ksw_extz2_sse)"""
    return ksw_extd2_batch(jobs, mat, gapo, gape, None, None)


def ksw_exts2_batch(jobs, mat, gapo, gape, gapo2, noncan):
    """splice-aware twin of ksw_extd2_batch (ksw_exts2_sse with junc == NULL); a job's w is ignored"""
    return ksw_extd2_batch(jobs, mat, gapo, gape, gapo2, None, noncan=noncan)


def ksw_extd2_batch(jobs, mat, gapo, gape, gapo2, gape2, noncan=None):
    """jobs: list of (query_bytes, target_bytes, w, zdrop, end_bonus, flag) with nt4 codes 0..4.
    Returns a list of (max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, cigar_tuple),
    the same tuple layout tests/reflib.py produces for the reference's ksw_extd2_sse."""
    n = len(jobs)
    arr = (KswJob * n)()
    keep = []
    tot = 0
    for i, (q, t, w, zdrop, end_bonus, flag) in enumerate(jobs):
        qb, tb = bytes(q), bytes(t)
        keep.append((qb, tb))
        arr[i].query = C.cast(C.c_char_p(qb), C.c_void_p)
        arr[i].target = C.cast(C.c_char_p(tb), C.c_void_p)
        arr[i].qlen, arr[i].tlen, arr[i].w, arr[i].zdrop, arr[i].end_bonus, arr[i].flag = len(qb), len(tb), w, zdrop, end_bonus, flag
        tot += len(qb) + len(tb)
    res = (KswRes * n)()
    pool = (C.c_uint32 * max(tot, 1))()
    if noncan is not None:
        _check(lib().mm2amd_ksw_exts2_batch(n, arr, 5, bytes(mat), gapo, gape, gapo2, noncan, res, pool, max(tot, 1)))
    elif gapo2 is None:
        _check(lib().mm2amd_ksw_extz2_batch(n, arr, 5, bytes(mat), gapo, gape, res, pool, max(tot, 1)))
    else:
        _check(lib().mm2amd_ksw_extd2_batch(n, arr, 5, bytes(mat), gapo, gape, gapo2, gape2, res, pool, max(tot, 1)))
    out = []
    for r in res:
        out.append((r.max, r.zdropped, r.max_q, r.max_t, r.mqe, r.mqe_t, r.mte, r.mte_q, r.score, r.reach_end,
                    tuple(pool[r.cigar_off:r.cigar_off + r.n_cigar])))
    return out


# ---------------------------------------------------------------------------------------------------------
# mappy-shaped front end
# ---------------------------------------------------------------------------------------------------------
_CODE_TO_BASE = bytes(b"ACGTN"[min(c, 4)] for c in range(256))


class Alignment(object):
    """One hit; field names follow mappy.Alignment (python/mappy.pyx:30-90)."""
    __slots__ = ("ctg", "ctg_len", "r_st", "r_en", "q_st", "q_en", "strand", "mapq", "is_primary", "mlen", "blen", "NM",
                 "cigar", "score", "dp_score", "rid", "sam_pri", "div", "parent", "id", "cs", "MD", "ds")

    @property
    def cigar_str(self):
        return "".join("%d%s" % (c >> 4, "MIDNSHP=XB"[c & 0xf]) for c in self.cigar)

    def key(self):
        """Everything the SAM/PAF writer reads from mm_reg1_t for this hit, as a comparable tuple."""
        return (self.rid, self.r_st, self.r_en, self.q_st, self.q_en, self.strand, self.mapq, self.is_primary, self.sam_pri,
                self.mlen, self.blen, self.score, self.dp_score, self.parent, self.id, tuple(self.cigar))


def _regs_to_alignments(n, regs, names, lens):
    out = []
    for j in range(n):
        r = regs[j]
        a = Alignment()
        a.rid, a.ctg, a.ctg_len = r.rid, names[r.rid] if names else None, lens[r.rid] if lens else None
        a.r_st, a.r_en, a.q_st, a.q_en = r.rs, r.re, r.qs, r.qe
        a.strand = -1 if r.rev else 1
        a.mapq, a.is_primary, a.sam_pri = r.mapq, int(r.id == r.parent), r.sam_pri
        a.mlen, a.blen, a.score, a.div, a.parent, a.id = r.mlen, r.blen, r.score, r.div, r.parent, r.id
        a.cs = a.MD = a.ds = ""  # filled on request (Aligner.map_batch(cs=, MD=, ds=)), as mappy's
        if r.p:
            ex = r.p.contents
            a.dp_score = ex.dp_score
            cig = C.cast(C.addressof(ex) + C.sizeof(Extra), C.POINTER(C.c_uint32 * ex.n_cigar)).contents if ex.n_cigar else ()
            a.cigar = list(cig)
            a.NM = r.blen - r.mlen + (ex.n_ambi_strand & 0x3fffffff)
        else:
            a.dp_score, a.cigar, a.NM = 0, [], 0
        out.append(a)
    return out


class _PoolItems(object):
    """Batch.items over records that point into a pool: (name, sequence) pairs made on request"""

    def __init__(self, arr, n):
        self.arr, self.n = arr, n

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(self.n))]
        if k < 0:
            k += self.n
        if not 0 <= k < self.n:
            raise IndexError(k)
        r = self.arr[k]
        return (r.name, C.string_at(r.seq, r.l_seq))


class Batch(object):
    """A mini-batch of reads as the reference's reader hands it to the mapping step: an array of mm_bseq1_t records over host buffers
    (bseq.h:14-17) plus the fragment table (seg_off, n_seg; map.c:560-575).  reads: list of (name, sequence), of sequences, or of
    (name, sequence1, sequence2) for read pairs.  Building one is the reader's work, not part of the hand-over."""

    def __init__(self, reads=None):
        self.n = 0
        self.items, self.arr, self.seg_off, self.n_seg = [], None, None, None
        if reads is None:
            return
        self.n = len(reads)
        seg_off, n_seg = [], []
        for i, r in enumerate(reads):
            r = r if isinstance(r, tuple) else ("read%d" % i, r)
            nb = r[0].encode() if isinstance(r[0], str) else r[0]
            seg_off.append(len(self.items)), n_seg.append(len(r) - 1)
            for q in r[1:]:
                self.items.append((nb, q.encode() if isinstance(q, str) else bytes(q)))
        self.arr = (Bseq1 * max(1, len(self.items)))()
        for k, (nb, sb) in enumerate(self.items):
            self.arr[k].l_seq, self.arr[k].rid, self.arr[k].name, self.arr[k].seq = len(sb), k, nb, sb
        self.seg_off, self.n_seg = (C.c_int * max(1, self.n))(*seg_off), (C.c_int * max(1, self.n))(*n_seg)
        self.bases = sum(len(sb) for _, sb in self.items)

    @classmethod
    def from_pool(cls, records, keep, seg_off, n_seg):
        """A batch over records that already lie in memory as mm_bseq1_t (FastxReader): records a numpy array with the fields of mm_bseq1_t whose
        name / seq / qual / comment hold addresses inside the buffers of `keep`, which the batch keeps alive; seg_off / n_seg numpy int32 arrays."""
        import numpy as np
        b = cls()
        records, seg_off, n_seg = np.ascontiguousarray(records), np.ascontiguousarray(seg_off, dtype=np.int32), np.ascontiguousarray(n_seg, dtype=np.int32)
        assert records.dtype.itemsize == C.sizeof(Bseq1)
        b.n, b._keep, b.records = len(seg_off), (keep, seg_off, n_seg), records
        m = len(records)
        b.arr = (Bseq1 * m).from_buffer(records) if m else (Bseq1 * 1)()
        b.seg_off = (C.c_int * b.n).from_buffer(seg_off) if b.n else (C.c_int * 1)()
        b.n_seg = (C.c_int * b.n).from_buffer(n_seg) if b.n else (C.c_int * 1)()
        b.items = _PoolItems(b.arr, m)
        b.bases = int(records["l_seq"].sum()) if m else 0
        return b

    def rotated(self, k):
        """the same reads starting at fragment k (fragments k.., then 0..k-1): new record and fragment tables over the SAME sequence
        buffers, made with two memmoves -- what a reader producing that order would have handed over"""
        if self.n == 0 or k % self.n == 0:
            return self
        k %= self.n
        b = Batch()
        b.n, b.items, b.bases = self.n, self.items, self.bases  # (items keeps the byte strings alive)
        m = len(self.items)
        first = self.seg_off[k]  # records of fragments k.. start here
        b.arr = (Bseq1 * max(1, m))()
        sz = C.sizeof(Bseq1)
        C.memmove(b.arr, C.byref(self.arr, first * sz), (m - first) * sz)
        C.memmove(C.byref(b.arr, (m - first) * sz), self.arr, first * sz)
        import numpy as np
        ns = np.frombuffer(self.n_seg, dtype=np.int32, count=self.n)
        ns = np.concatenate([ns[k:], ns[:k]])
        so = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int32)
        b.n_seg, b.seg_off = (C.c_int * self.n).from_buffer_copy(ns.tobytes()), (C.c_int * self.n).from_buffer_copy(so.tobytes())
        return b


class Aligner(object):
    """Index built on the GPU from in-memory sequences + batched mapping; mirrors mappy.Aligner(seq=..., preset=...).

    seq: a sequence string/bytes or a list of them (the reference); names: optional list of contig names.
    fn_idx_in: instead of seq, a file -- a minimap2 index (.mmi, read by mm2amd_idx_load; part: which part of a multi-part file, required when
    there is more than one; the file's k, w and flags replace the preset's) or FASTA / FASTQ, plain or gzip.  fn_idx_out: write the index there
    as a .mmi (mm2amd_idx_dump) once it is built.  extra_flags: MM_F_* bits ORed into map_opt.flag (mappy's parameter of the same name).
    sdust_thres: minimap2's -T (minimizers lying mostly in SDUST-masked stretches of a read are dropped; 0 = off).  eqx: minimap2's --eqx (MM_F_EQX).
    write_junc: minimap2's --write-junc (MM_F_OUT_JUNC | MM_F_CIGAR): the text of pipeline(text=True), format_raw() and map_pairs(text=True) is then
    the splice junctions of the hits (one BED-like line per intron; the input of a second pass with --pass1) instead of SAM / PAF records.
    n_gpus / device_ids: map every batch on several GPUs of this process (mm_gpu_init_index_multi: index replicated, reads sharded
    by bases; an ordinal may repeat).  Only one Aligner can be the active mapper of the process at a time (the drop-in boundary is
    a process-wide context, like the reference's pipeline): creating a second one makes the first inactive -- its map calls raise,
    and closing or collecting it leaves the new context alone."""

    def __init__(self, seq=None, preset=None, names=None, k=None, w=None, n_threads=0, cigar=True, sam=False, n_gpus=0, device_ids=None,
                 fn_idx_in=None, fn_idx_out=None, part=None, extra_flags=0, sdust_thres=0, eqx=False, write_junc=False, split_prefix=None, opt_overrides=None):
        L = lib()
        self._generation, self._idx, self._staged = 0, None, None  # close() must work on a half-built object
        self.last_format_path = None  # FMT_PATH_* of the last format_raw(device=True)
        if (seq is None) == (fn_idx_in is None):
            raise Mm2AmdError("give exactly one of seq and fn_idx_in")
        self.idx_opt, self.map_opt = IdxOpt(), MapOpt()
        L.mm2amd_set_opt(None, C.byref(self.idx_opt), C.byref(self.map_opt))
        if preset is not None and L.mm2amd_set_opt(preset.encode(), C.byref(self.idx_opt), C.byref(self.map_opt)) != 0:
            raise Mm2AmdError("unknown preset %r" % preset)
        if k:
            self.idx_opt.k = k
        if w:
            self.idx_opt.w = w
        if cigar:
            self.map_opt.flag |= F_CIGAR
        if sam:
            self.map_opt.flag |= F_OUT_SAM | F_CIGAR
        self.map_opt.flag |= extra_flags  # MM_F_* bits beyond the preset's (mappy.Aligner's extra_flags)
        if eqx:
            self.map_opt.flag |= F_EQX  # minimap2's --eqx
        if write_junc:
            self.map_opt.flag |= F_OUT_JUNC | F_CIGAR  # minimap2's --write-junc (main.c)
        if sdust_thres:
            self.map_opt.sdust_thres = sdust_thres
        for name, value in (opt_overrides or {}).items():  # fields of mm_mapopt_t by name, e.g. {"best_n": 20, "pri_ratio": 0.3} for -N 20 -p 0.3
            setattr(self.map_opt, name, value)
        if split_prefix is not None:  # minimap2's --split-prefix: the first pass over one part of a multi-part index (map_split)
            self._split_prefix = os.fsencode(split_prefix)
            self.map_opt.split_prefix = self._split_prefix
        from_index = fn_idx_in is not None and idx_is_idx(fn_idx_in)
        if from_index:
            # a prebuilt index: its k, w and flag win over the preset's, as in the reference's reader (mm_idx_reader_read, index.c:621-635)
            self._idx, more = idx_load(fn_idx_in, part or 0)
            self.more_parts = more  # another part follows this one in the file
            if more and part is None:
                raise Mm2AmdError("%s holds more than one index part: say which with part=" % fn_idx_in)
            st = self.index_stat()
            self.idx_opt.k, self.idx_opt.w, self.idx_opt.flag = st["k"], st["w"], st["flag"]
            self._seqs = None
            nm, ln = C.c_char_p(), C.c_uint32()
            self.names, self.lens = [], []
            for i in range(st["n_seq"]):
                _check(L.mm2amd_idx_seq(self._idx, i, C.byref(nm), C.byref(ln)))
                self.names.append(nm.value.decode() if nm.value is not None else None)
                self.lens.append(ln.value)
            self._name_bytes = None
        else:
            if fn_idx_in is not None:  # FASTA / FASTQ, plain or gzip
                if part:
                    raise Mm2AmdError("part= applies to index files")
                file_names, seq = read_fastx(fn_idx_in)
                names = names or file_names
            seqs = [seq] if isinstance(seq, (bytes, str)) else list(seq)
            self._seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
            n = len(self._seqs)
            self.names = [x if isinstance(x, str) else x.decode() for x in names] if names else ["ref%d" % i for i in range(n)]
            self.lens = [len(s) for s in self._seqs]
        _check(L.mm2amd_check_opt(C.byref(self.idx_opt), C.byref(self.map_opt)))
        if not from_index:
            sarr = (C.c_char_p * n)(*self._seqs)
            self._name_bytes = [x.encode() for x in self.names]
            narr = (C.c_char_p * n)(*self._name_bytes)
            self._idx = L.mm2amd_idx_str(self.idx_opt.w, self.idx_opt.k, self.idx_opt.flag & 1, self.idx_opt.bucket_bits, n, sarr, narr)
            if not self._idx:
                raise Mm2AmdError("index construction failed: %s" % L.mm2amd_last_error().decode())
        if fn_idx_out is not None:
            idx_dump(self._idx, fn_idx_out, self.idx_opt.bucket_bits, DUMP_NO_SEQ if self.index_stat()["flag"] & I_NO_SEQ else 0)
        _check(L.mm2amd_mapopt_update(C.byref(self.map_opt), self._idx))
        ids = (C.c_int * len(device_ids))(*device_ids) if device_ids else None
        _check(L.mm_gpu_init_index_multi(self._idx, C.byref(self.map_opt), n_threads, len(device_ids) if device_ids else n_gpus, ids))
        self._generation = L.mm_gpu_context_generation()
        self._staged = None

    @property
    def seq_names(self):
        """the reference sequences' names, in index order (mappy.Aligner.seq_names)"""
        return list(self.names)

    def _active(self):
        if lib().mm_gpu_context_generation() != self._generation:
            raise Mm2AmdError("this Aligner is no longer the process's active mapper (a later Aligner or mm_gpu_init replaced its context)")

    def close(self):
        if getattr(self, "_idx", None):
            lib().mm_gpu_destroy_if(self._generation)  # only the context this object installed
            lib().mm2amd_idx_destroy(self._idx)
            self._idx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def index_stat(self):
        k, w, flag, n_seq = C.c_int(), C.c_int(), C.c_int(), C.c_uint32()
        sl, nd, nm = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().mm2amd_idx_stat(self._idx, k, w, flag, n_seq, sl, nd, nm))
        return {"k": k.value, "w": w.value, "flag": flag.value, "n_seq": n_seq.value, "sum_len": sl.value,
                "n_distinct": nd.value, "n_minimizers": nm.value}

    # -- batch interface: stage() + run() == map_batch() ------------------------------------------------
    def stage(self, reads):
        """reads: list of (name, sequence), of sequences (bytes/str), or of (name, sequence1, sequence2) for read pairs (mapped as
        two-segment fragments, mm_map_frag with n_segs == 2), or a Batch.  Copies them to the GPU."""
        self._active()
        b = reads if isinstance(reads, Batch) else Batch(reads)
        _check(lib().mm_gpu_batch_stage(b.n, b.seg_off, b.n_seg, b.arr))
        self._staged = (b.n, b.arr, b.items, b.seg_off, b.n_seg)

    def pipeline(self, batches, text=True, on_mapped=None, on_text=None, trace=None):
        """The reference's three-step pipeline (map.c:541-643) over an iterable of Batch objects, every step on a thread of its own so
        that the steps of successive batches overlap: hand-over (mm_gpu_batch_stage_queued: pack + H2D beside the mapping of the batch
        before), mapping (mm_gpu_map_staged), output stage (mm_gpu_format_batch_view: SAM / PAF text of the batch in a reused buffer).
        on_mapped(batch, n_reg, reg, rep_len) runs on the output thread before formatting (e.g. the multi-GPU hit gather);
        on_text(batch, address, length) receives the text (valid until the next batch's).  Hit records are freed after on_text.
        trace: a list that receives (step, batch number, start, end) wall-clock intervals of the three steps.
        Returns the number of text bytes produced."""
        import queue
        import threading
        import time
        self._active()
        L = lib()
        q_staged, q_mapped = queue.Queue(maxsize=2), queue.Queue(maxsize=2)
        errors, total = [], [0]

        def stager():
            try:
                for k, b in enumerate(batches):
                    if errors:
                        break
                    t0 = time.time()
                    _check(L.mm_gpu_batch_stage_queued(b.n, b.seg_off, b.n_seg, b.arr))
                    if trace is not None:
                        trace.append(("stage", k, t0, time.time()))
                    q_staged.put(b)
            except Exception as e:  # noqa: BLE001
                errors.append(e)
            q_staged.put(None)

        def mapper():
            try:
                k = 0
                while True:
                    b = q_staged.get()
                    if b is None:
                        break
                    m = max(1, len(b.items))
                    n_reg, reg, rep_len, frag_gap = (C.c_int * m)(), (C.c_void_p * m)(), (C.c_int * m)(), (C.c_int * m)()
                    t0 = time.time()
                    _check(L.mm_gpu_map_staged(n_reg, reg, rep_len, frag_gap))
                    if trace is not None:
                        trace.append(("map", k, t0, time.time()))
                    k += 1
                    q_mapped.put((b, n_reg, reg, rep_len))
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                while True:  # let the stager finish: its staged batches are dropped
                    L.mm_gpu_batch_discard()
                    try:
                        if q_staged.get(timeout=0.05) is None:
                            break
                    except queue.Empty:
                        pass
            q_mapped.put(None)

        def output():
            k = -1
            while True:
                it = q_mapped.get()
                if it is None:
                    break
                b, n_reg, reg, rep_len = it
                k += 1
                t0 = time.time()
                try:
                    if not errors:
                        if on_mapped:
                            on_mapped(b, n_reg, reg, rep_len)
                        if text:
                            out, out_len = C.c_void_p(), C.c_size_t()
                            _check(L.mm_gpu_format_batch_view(b.n, b.seg_off, b.n_seg, b.arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len)))
                            total[0] += out_len.value
                            if on_text:
                                on_text(b, out.value, out_len.value)
                except Exception as e:  # noqa: BLE001
                    errors.append(e)
                t1 = time.time()
                L.mm2amd_free_regs(len(n_reg), n_reg, reg)
                if trace is not None:
                    trace.append(("output", k, t0, t1)), trace.append(("free", k, t1, time.time()))

        def named(f, nm):  # the OS-level thread name (/proc/<pid>/task/*/comm): bench.py attributes CPU seconds by it
            def g():
                try:
                    C.CDLL(None).prctl(15, nm, 0, 0, 0)  # PR_SET_NAME
                except Exception:  # noqa: BLE001
                    pass
                f()
            return g
        th = [threading.Thread(target=named(f, nm)) for f, nm in ((stager, b"mm2-stager"), (mapper, b"mm2-mapper"), (output, b"mm2-output"))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        self._staged = None
        if errors:
            raise errors[0]
        return total[0]

    def run(self, raw=False, cs=False, MD=False, ds=False):
        """Maps the staged batch.  Returns one list of alignments per read, or a pair of lists for a read pair.  raw=True returns
        (n_reg, reg, rep_len) ctypes arrays (one entry per read, pairs adjacent) that must be passed to free_raw().
        cs / MD / ds: fill Alignment.cs (the short form) / Alignment.MD / Alignment.ds (the short form, mappy's mm_gen_ds with no_iden = 1) --
        one mm2amd_hits_text_batch call per tag over all hits of the batch."""
        if self._staged is None:
            raise Mm2AmdError("run() without stage()")
        self._active()
        n, _, items, seg_off, n_seg = self._staged
        m = max(1, len(items))
        n_reg, reg, rep_len, frag_gap = (C.c_int * m)(), (C.c_void_p * m)(), (C.c_int * m)(), (C.c_int * m)()
        _check(lib().mm_gpu_map_staged(n_reg, reg, rep_len, frag_gap))
        if raw:
            return n_reg, reg, rep_len
        out = []
        for i in range(n):
            per = []
            for k in range(seg_off[i], seg_off[i] + n_seg[i]):
                regs = C.cast(reg[k], C.POINTER(Reg1)) if n_reg[k] else None
                per.append(_regs_to_alignments(n_reg[k], regs, self.names, self.lens))
            out.append(per[0] if n_seg[i] == 1 else tuple(per))
        try:
            if cs or MD or ds:
                flat = [a for per in out for seg in (per if isinstance(per, tuple) else (per,)) for a in seg]  # read order, as the records below
                segs = [k for i in range(n) for k in range(seg_off[i], seg_off[i] + n_seg[i])]
                ptrs = [reg[k] + j * C.sizeof(Reg1) for k in segs for j in range(n_reg[k])]
                rds = [items[k][1] for k in segs for j in range(n_reg[k])]
                for want, what, field in ((cs, TXT_CS, "cs"), (MD, TXT_MD, "MD"), (ds, TXT_DS, "ds")):
                    if want and ptrs:
                        for a, t in zip(flat, hits_text(self._idx, ptrs, rds, what)):
                            setattr(a, field, t or "")
        finally:
            lib().mm2amd_free_regs(len(items), n_reg, reg)
        return out

    def free_raw(self, n_reg, reg):
        lib().mm2amd_free_regs(len(n_reg), n_reg, reg)

    def format_raw(self, n_reg, reg, rep_len=None, device=False):
        """SAM (or PAF, by the aligner's options) records of the staged batch's raw results, as bytes: what the reference's
        output step writes for these reads (mm_gpu_format_batch).  device=True: the records are written on the device
        (mm_gpu_format_batch_dev); last_format_path then says who wrote them (FMT_PATH_DEVICE, or FMT_PATH_HOST for a batch the
        device path leaves to the host writer)."""
        n, arr, _, seg_off, n_seg = self._staged
        out, out_len = C.c_void_p(), C.c_size_t()
        if device:
            path = C.c_int(-1)
            _check(lib().mm_gpu_format_batch_dev(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len), C.byref(path)))
            self.last_format_path = path.value
            return C.string_at(out, out_len.value)  # (the library owns the buffer)
        _check(lib().mm_gpu_format_batch(n, seg_off, n_seg, arr, n_reg, reg, rep_len, C.byref(out), C.byref(out_len)))
        try:
            return C.string_at(out, out_len.value)
        finally:
            _libc_free(out)

    def map_batch(self, reads, cs=False, MD=False, ds=False):
        self.stage(reads)
        return self.run(cs=cs, MD=MD, ds=ds)

    def map(self, seq, seq2=None, name="query", cs=False, MD=False, ds=False):
        """Single-read (or, with seq2, single-pair) convenience wrapper (mappy.Aligner.map); a batch of one."""
        if seq2 is not None:
            return self.map_pairs([(name, seq, seq2)], cs=cs, MD=MD, ds=ds)[0]
        return self.map_batch([(name, seq)], cs=cs, MD=MD, ds=ds)[0]

    def seq(self, name, start=0, end=0x7fffffff):
        """mappy.Aligner.seq (python/mappy.pyx:239, cmappy.h:122-138): bases [start, end) of the named reference sequence as str, end clipped
        to the sequence; None for an unknown name, an empty range or an index without sequence (mm2amd_idx_getseq)."""
        if not self._idx or self.index_stat()["flag"] & I_NO_SEQ or name not in self.names:
            return None
        rid = self.names.index(name)
        if start < 0 or start >= self.lens[rid] or start >= end:
            return None
        end = min(end, self.lens[rid])
        buf = C.create_string_buffer(end - start)
        rc = lib().mm2amd_idx_getseq(self._idx, rid, start, end, buf)
        if rc < 0:
            _check(rc)
        return buf.raw.translate(_CODE_TO_BASE).decode("ascii")

    def map_pairs(self, pairs, text=False, cs=False, MD=False, ds=False):
        """Paired-end reads: pairs = list of (name, seq1, seq2) (use preset "sr").  Returns a list of (alignments of read 1,
        alignments of read 2), with cs / MD / ds filled on request; with text=True the SAM/PAF records of the batch instead
        (mm_gpu_format_batch, mate fields included)."""
        self.stage(pairs)
        if not text:
            return self.run(cs=cs, MD=MD, ds=ds)
        n_reg, reg, rep_len = self.run(raw=True)
        try:
            return self.format_raw(n_reg, reg, rep_len)
        finally:
            self.free_raw(n_reg, reg)

    def last_stats(self):
        v = (C.c_double * 48)()
        k = lib().mm2amd_last_stats(v, 48)
        names = ["t_seed_chain", "t_host_pre", "t_plan", "t_ksw", "t_consume", "t_finish", "n_jobs", "n_rounds", "dp_cells", "dev_allocs", "pin_allocs",
                 "alloc_ns", "cpu_seed_chain", "cpu_host_pre", "cpu_plan", "cpu_ksw", "cpu_consume", "cpu_finish", "n_long_join_dev", "n_long_join_host",
                 "drv_cpu_seed_chain", "drv_cpu_host_pre", "drv_cpu_plan", "drv_cpu_ksw", "drv_cpu_consume", "drv_cpu_finish", "n_early_sub",
                 "n_region_reads_dev", "n_region_reads_host", "n_band128", "n_band256", "n_band_widened", "n_band_rectangle",
                 "arena_dev_bytes", "arena_pin_bytes", "arena_dev_used", "arena_pin_used", "n_band512", "n_band_rectangle_big",
                 "n_anchors_prune_in", "n_anchors_prune_kept", "n_reads_prune_redo"]  # (the last three: process-wide since start, like the band counters)
        return dict(zip(names, list(v)[:k]))


class SplitWriter(object):
    """The temp file PREFIX.NNNN.tmp of minimap2's --split-prefix for one index part (mm2amd_split_open / _write / _close): what the reference's
    first pass writes (splitidx.c:8-31, map.c:589-600), for its mm_split_merge or for SplitMerger to read."""

    def __init__(self, prefix, aligner, part_no):
        self._al, self._h = aligner, None
        self._h = lib().mm2amd_split_open(os.fsencode(prefix), aligner._idx, part_no)
        if not self._h:
            _check(lib().mm2amd_last_error_code())

    def write(self, n_seq, n_reg, reg, rep_len, frag_gap):
        """the raw results of a mapped batch of n_seq read segments"""
        _check(lib().mm2amd_split_write(self._h, C.byref(self._al.map_opt), n_seq, n_reg, reg, rep_len, frag_gap))

    def close(self):
        if self._h:
            h, self._h = self._h, None
            _check(lib().mm2amd_split_close(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SplitMerger(object):
    """The merge pass of minimap2's --split-prefix over the temp files of n_parts parts (mm2amd_split_merge_*; mm_split_merge, map.c:693-736).
    map_opt: the MapOpt of the first pass (after mm_mapopt_update).  MM2AMD_DEVICE_MERGE=1 sends the hit-list rules through hits_merge_kernel."""

    def __init__(self, prefix, n_parts, map_opt):
        self._h = lib().mm2amd_split_merge_open(os.fsencode(prefix), n_parts, C.byref(map_opt))
        if not self._h:
            _check(lib().mm2amd_last_error_code())

    def sq_lines(self):
        """the @SQ lines of all parts, in part order"""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().mm2amd_split_merge_sq(self._h, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            _libc_free(out)

    def merge(self, batch):
        """the next mini-batch of reads, in file order -> (n_reg, reg, rep_len, frag_gap), to be freed with mm2amd_free_regs"""
        m = max(1, len(batch.items))
        n_reg, reg, rep_len, frag_gap = (C.c_int * m)(), (C.c_void_p * m)(), (C.c_int * m)(), (C.c_int * m)()
        _check(lib().mm2amd_split_merge_batch(self._h, batch.n, batch.seg_off, batch.n_seg, batch.arr, n_reg, reg, rep_len, frag_gap))
        return n_reg, reg, rep_len, frag_gap

    def format(self, batch, n_reg, reg, rep_len):
        """SAM / PAF records of a merged batch, as bytes"""
        out, n = C.c_void_p(), C.c_size_t()
        _check(lib().mm2amd_split_merge_format(self._h, batch.n, batch.seg_off, batch.n_seg, batch.arr, n_reg, reg, rep_len, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            _libc_free(out)

    def close(self, remove_tmp=True):
        if self._h:
            h, self._h = self._h, None
            _check(lib().mm2amd_split_merge_close(h, 1 if remove_tmp else 0))

    def __del__(self):
        try:
            self.close(False)
        except Exception:
            pass


def map_split(fn_idx, read_files, split_prefix, out, preset=None, sam=True, batch_bases=500_000_000, idx_batch_size=8_000_000_000, pg_line=None, keep_tmp=False, cs=False, MD=False, ds=False,
              **aligner_options):
    """minimap2's --split-prefix: map the reads of read_files (a file name, or a list of two for read pairs) against every part of fn_idx -- a
    multi-part .mmi, or a FASTA / FASTQ cut into chunks of idx_batch_size bases (minimap2's -I) -- one part at a time, writing the part's temp file and freeing the part; then write
    the header (with sam=True: @HD, the @SQ lines of all parts, pg_line if given), merge, format and remove the temp files.  out: a file name or
    a binary file object.  aligner_options go to Aligner (n_threads, extra_flags, ...).  Returns the number of parts."""
    L = lib()
    files = [read_files] if isinstance(read_files, (str, bytes)) else list(read_files)
    flags = aligner_options.pop("extra_flags", 0) | (0x040 if cs else 0) | (0x1000000 if MD else 0) | (0x2000000000 if ds else 0)  # MM_F_OUT_CS / _MD / _DS
    if flags & (0x040 | 0x1000000 | 0x2000000000 | F_OUT_JUNC) or aligner_options.get("write_junc"):
        e = Mm2AmdError("mm2amd error %d: --cs, --MD, --ds and --write-junc do not work with --split-prefix" % EINVAL)
        e.code = EINVAL
        raise e
    multi = idx_is_idx(fn_idx)
    chunks = None if multi else iter(FastxReader(fn_idx, chunk_bases=idx_batch_size, with_qual=False))  # a sequence file: -I-sized chunks, as mm_idx_gen reads them
    nxt = None if multi else next(chunks, None)
    n_parts, map_opt = 0, None
    try:
        while True:
            if multi:
                al = Aligner(fn_idx_in=fn_idx, part=n_parts, preset=preset, sam=sam, extra_flags=flags, split_prefix=split_prefix, **aligner_options)
            else:
                if nxt is None:
                    raise Mm2AmdError("%s holds no sequence" % fn_idx)
                cur, nxt = nxt, next(chunks, None)
                al = Aligner(seq=[q for _, q in cur.items], names=[nm.decode() for nm, _ in cur.items], preset=preset, sam=sam, extra_flags=flags, split_prefix=split_prefix,
                             **aligner_options)
                del cur
            try:
                more = al.more_parts if multi else nxt is not None
                w = SplitWriter(split_prefix, al, n_parts)
                try:
                    rd = FastxReader(files if len(files) > 1 else files[0], chunk_bases=batch_bases, frag_mode=bool(al.map_opt.flag & F_FRAG_MODE))
                    for b in rd:
                        al.stage(b)
                        m = max(1, len(b.items))
                        n_reg, reg, rep_len, frag_gap = (C.c_int * m)(), (C.c_void_p * m)(), (C.c_int * m)(), (C.c_int * m)()
                        _check(L.mm_gpu_map_staged(n_reg, reg, rep_len, frag_gap))
                        try:
                            w.write(len(b.items), n_reg, reg, rep_len, frag_gap)
                        finally:
                            L.mm2amd_free_regs(len(n_reg), n_reg, reg)
                    rd.close()
                finally:
                    w.close()
                map_opt = MapOpt.from_buffer_copy(al.map_opt)
            finally:
                al.close()
            n_parts += 1
            if not more:
                break
        keep = os.fsencode(split_prefix)
        map_opt.split_prefix = keep
        mg = SplitMerger(split_prefix, n_parts, map_opt)
        f = open(out, "wb") if isinstance(out, (str, bytes)) else out
        try:
            if sam:
                f.write(b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + mg.sq_lines() + (pg_line or b""))
            rd = FastxReader(files if len(files) > 1 else files[0], chunk_bases=batch_bases, frag_mode=bool(map_opt.flag & F_FRAG_MODE))
            for b in rd:
                n_reg, reg, rep_len, _ = mg.merge(b)
                try:
                    f.write(mg.format(b, n_reg, reg, rep_len))
                finally:
                    L.mm2amd_free_regs(len(n_reg), n_reg, reg)
            rd.close()
        finally:
            if f is not out:
                f.close()
            mg.close(remove_tmp=not keep_tmp)
    except Exception:
        if not keep_tmp:
            for j in range(n_parts + 1):
                try:
                    os.remove("%s.%.4d.tmp" % (split_prefix, j))
                except OSError:
                    pass
        raise
    return n_parts


def band_counters():
    """The banded gap-fill kernel's windows since the process started (ksw_band.hip): tried in a band of 128 / 256 diagonals, sent on to the wider band,
    computed again as full rectangles.  (Zeros in a library without the kernels.)"""
    L = lib()
    if not hasattr(L, "mm2amd_alloc_counter"):
        return {"band128": 0, "band256": 0, "widened": 0, "rectangle": 0, "band512": 0, "rectangle_big": 0}
    L.mm2amd_alloc_counter.restype = C.c_longlong
    L.mm2amd_alloc_counter.argtypes = [C.c_int]
    return {"band128": L.mm2amd_alloc_counter(3), "band256": L.mm2amd_alloc_counter(4), "widened": L.mm2amd_alloc_counter(5), "rectangle": L.mm2amd_alloc_counter(6),
            "band512": L.mm2amd_alloc_counter(11), "rectangle_big": L.mm2amd_alloc_counter(12)}


def profile_enable(on=True):
    lib().mm2amd_profile_enable(1 if on else 0)


def profile_get():
    arr = (KernelStat * 64)()
    n = lib().mm2amd_profile_get(arr, 64)
    return {arr[i].name.decode(): {"ms": arr[i].ms, "alg_bytes": arr[i].alg_bytes, "launches": arr[i].launches, "units": arr[i].units} for i in range(n)}
