"""phfpfac_amd -- MI355X-native PFAC (Parallel Failureless Aho-Corasick) multi-pattern matcher.

Host side (C, ``csrc/pfac_table.c``) builds the perfect-hash-compressed state-transition table;
the scan runs in a hand-written gfx950 HIP kernel (``csrc/pfac_hip.hip``) behind the C-ABI of
``include/pfac.h``.  This package is the thin Python mirror of that ABI plus the
``torch.distributed`` plumbing that shards the input byte stream across GPUs.
"""
from ._ffi import PFAC_COUNT_ACCUMULATE, PFAC_TERMS_SELECTION, PFAC_TOKEN_DROP, PFAC_TOKENS_POSITIONS, PfacError  # noqa: F401
from ._ffi import PFAC_LINE_CONTEXT_SEP, PFAC_LINE_NUMBER, PFAC_LINE_OFFSET, PFAC_LINE_SEP_FIRST, PFAC_LINE_TERMINATE  # noqa: F401
from .table import RECORD_DTYPE, SCORE_DTYPE, SPAN_DTYPE, PfacTable, emit_packed, emit_records, emit_records_multi, fold_ascii, merge_partitions, replacement_table, strip_anchors, template_table, token_table, wordpiece_table  # noqa: F401
from ._ffi import PFAC_NEAR_ANY_DIST, PFAC_NEAR_MAX_RULES, PFAC_NEAR_ORDERED, PFAC_NEAR_SELECTION  # noqa: F401
from .table import NEAR_RULE_DTYPE, near_rule  # noqa: F401
from .table import UNIGRAM_PIECE_DTYPE, unigram_table  # noqa: F401
from .table import BPE_PIECE_DTYPE, bpe_byte_alphabet, bpe_table  # noqa: F401
from ._ffi import PFAC_RULE_NOT  # noqa: F401
from .matcher import GpuMatcher, device_count, word_set  # noqa: F401

__all__ = ["PfacError", "PfacTable", "GpuMatcher", "RECORD_DTYPE", "emit_records", "emit_packed", "emit_records_multi", "merge_partitions", "replacement_table", "fold_ascii", "device_count", "word_set", "PFAC_COUNT_ACCUMULATE", "SPAN_DTYPE", "SCORE_DTYPE", "strip_anchors", "template_table", "PFAC_TERMS_SELECTION", "token_table", "wordpiece_table", "PFAC_TOKEN_DROP", "PFAC_TOKENS_POSITIONS", "NEAR_RULE_DTYPE", "near_rule", "PFAC_NEAR_MAX_RULES", "PFAC_NEAR_ORDERED", "PFAC_NEAR_ANY_DIST",
           "PFAC_NEAR_SELECTION", "PFAC_RULE_NOT", "unigram_table", "UNIGRAM_PIECE_DTYPE", "bpe_table", "bpe_byte_alphabet", "BPE_PIECE_DTYPE"]
