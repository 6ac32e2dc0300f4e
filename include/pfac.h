/*
 * include/pfac.h -- C-ABI of the MI355X-native PFAC matcher.
 *
 * Two shared libraries implement it:
 *   libpfac_host.so  (plain C, no GPU)  : pattern file -> PHF-compressed state-transition table
 *   libpfac_hip.so   (HIP, gfx950)      : device contexts, table upload, the scan kernel, records
 *
 * Every entry point below names the reference interface it replaces
 * (paths relative to mickeyjoe666/PHFPFAC regex_GPU_PHF/).  The reference has
 * no FFI: main.cc calls three C++-linkage functions (main.cc:35-37) and
 * #includes its table builder (main.cc:5-6).  A maintainer switches to this
 * library by replacing those call sites; see INTEGRATION.md.
 *
 * Conventions: plain pointers and integers only; every function returns 0 on
 * success or a negative pfac_status; nothing calls exit() (the reference exits
 * on every error, e.g. master_kernel.cu:240-244).  No function falls back to
 * a CPU implementation: without a usable GPU the HIP library reports
 * PFAC_E_NO_DEVICE / PFAC_E_HIP.
 */
#ifndef PFAC_H
#define PFAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PFAC_OK = 0,
    PFAC_E_ARG = -1,        /* bad argument (NULL, misaligned pointer, width not a power of two <= 4096, ...) */
    PFAC_E_IO = -2,         /* cannot open / read a file */
    PFAC_E_PATTERN = -3,    /* pattern file violates the reader's rules (length >= 1024, empty line, no trailing '\n') */
    PFAC_E_NOMEM = -4,
    PFAC_E_NO_DEVICE = -5,  /* no HIP device / bad device index */
    PFAC_E_HIP = -6,        /* a HIP runtime call failed; see pfac_last_error() */
    PFAC_E_STATE = -7,      /* call order violated (scan before table upload, ...) */
    PFAC_E_OVERFLOW = -8,   /* more matches than the record buffer holds (count is still exact) */
    PFAC_E_INTERNAL = -9    /* kernel reported an internal fault (a bounded wait of the scan protocol timed out) */
} pfac_status;

/* ------------------------------------------------------------------ */
/* Host side (libpfac_host.so): the CreateTable/ + PHF/ path.          */

/*
 * The PHF-compressed transition table in the reference's own terms
 * (struct thread_data, main.cc:19-32 / master_kernel.cu:15-28):
 *   s0[256]          root row  PFAC[initial_state][*]            (main.cc:200)
 *   r[max_row]       row displacement, may be negative, -1 empty (phf.c:67,197)
 *   HT[ht_size]      owning row of each slot, -1 free            (phf.c:211)
 *   val[ht_size]     next state of each slot                     (phf.c:216)
 *   idmap[num_final] final state -> pattern id (1-based line no) (create_table_reorder.c:318)
 * lookup(state, ch): key=(state<<8)+ch; row=key>>width_bit; col=key&(width-1);
 *   idx=r[row]+col; 0<=idx<ht_size && HT[idx]==row ? val[idx] : -1   (master_kernel.cu:52-63)
 * States: finals are 0..num_final-1 (index in the sorted pattern list), the
 * root is num_final+1, internal states follow (create_table_reorder.c:287-292).
 * Unlike the reference, ONE automaton covers the whole pattern file: the
 * 4*streamnum pattern chunks (create_table_reorder.c:217) are not needed
 * because the input, not the pattern set, is what gets sharded.
 */
typedef struct pfac_table {
    int32_t width;          /* power of two, 1 <= width <= 4096 (phf.c:8,161) */
    int32_t width_bit;      /* log2(width) (master_kernel.cu:397-398) */
    int32_t n_patterns;     /* lines in the pattern file */
    int32_t num_final;      /* == n_patterns (duplicates keep their own, unreachable, final state) */
    int32_t state_num;
    int32_t max_pat_len;
    int32_t max_row;        /* entries in r   = (state_num*256)/width + 1 (master_kernel.cu:212) */
    int32_t ht_size;        /* entries in HT and val */
    int32_t n_keys;         /* transitions stored */
    int32_t *s0;
    int32_t *r;
    int32_t *HT;
    int32_t *val;
    int32_t *idmap;
} pfac_table;

/* Replaces create_PFAC_table_reorder() + FFDM() (main.cc:108,125):
 * read_pattern (create_table_reorder.c:53), sort (comp_pat :21), trie
 * (patternsToPFAC :277) and the row-displacement perfect hash (phf.c:151),
 * in near-linear time and without the 4 GiB-per-chunk preallocation. */
int pfac_table_build_file(const char *pattern_file, int width, pfac_table **out, char *err, size_t err_len);
/* Escape-aware variant: the reference's read_pattern_ext()/fgetc_ext() (create_table_reorder.c:131-185,
 * ctdef.h:37-99, dead code there): \a \b \t \n \v \f \r \' \" \\ \ooo \xNN inside patterns; only a real
 * newline separates patterns, so patterns may contain newline bytes.  Everything downstream is unchanged. */
int pfac_table_build_file_escaped(const char *pattern_file, int width, pfac_table **out, char *err, size_t err_len);
/* Same as pfac_table_build_file, from a memory image of a pattern file. */
int pfac_table_build_mem(const void *patterns, size_t n_bytes, int width, pfac_table **out, char *err, size_t err_len);
/* Pattern-partition mode -- the reference's own multi-GPU scheme (create_table_reorder.c:217-247), kept as a
 * fallback for automata that outgrow L2/MALL: the table of partition `part` of `n_parts` of the SORTED pattern
 * list (k = n / P patterns each, the last one also takes n % P; ids stay whole-file line numbers, max_pat_len
 * stays the global maximum).  A cut never separates identical lines, so duplicates resolve inside one
 * partition ("last line wins") instead of overflowing result slots as main.cc:308-315 does.  Every partition
 * scans the whole input; pfac_merge_partitions() below is the merge of main.cc:304-324. */
int pfac_table_build_file_part(const char *pattern_file, int width, int part, int n_parts, pfac_table **out, char *err,
                               size_t err_len);
int pfac_table_build_mem_part(const void *patterns, size_t n_bytes, int width, int part, int n_parts, pfac_table **out,
                              char *err, size_t err_len);
void pfac_table_free(pfac_table *t);

/* Character-class patterns -- the front end the reference sketches in CreateTable/charset_table_reorder.c:45-168,
 * 321-427 (orphaned and not compilable there): a pattern is a sequence of single (escape-aware) characters and classes
 * "[...]" / "[^...]" with "l-r" ranges; no repetition.  The subset construction yields an acyclic DFA that is used as
 * the PFAC table unchanged (finals first, root = num_final + 1).  A final state can stand for several patterns:
 * outputs->ids[outputs->first[s] .. outputs->first[s+1]) lists them, ascending; table->idmap[s] is the first one.
 * num_final counts FINAL STATES here, n_patterns the lines of the file.  Parity with the reference: unpinned (its code
 * for this cannot be built); pinned against an independent brute-force matcher (oracle/charclass_oracle.py). */
typedef struct pfac_outputs {
    int32_t n_states;       /* == table->num_final */
    int32_t *first;         /* [n_states + 1] */
    int32_t *ids;           /* pattern ids (1-based line numbers) */
} pfac_outputs;
int pfac_table_build_file_charclass(const char *pattern_file, int width, pfac_table **out, pfac_outputs **outputs, char *err,
                                    size_t err_len);
int pfac_table_build_mem_charclass(const void *patterns, size_t n_bytes, int width, pfac_table **out, pfac_outputs **outputs,
                                   char *err, size_t err_len);
void pfac_outputs_free(pfac_outputs *o);

/* Case-insensitive tables (grep -i, the `nocase` of Snort-style rules).  pfac_fold_ascii is THE fold, the one the scan
 * kernel applies under PFAC_FOLD_ASCII (pfac_table_set_case_fold): every byte 0x41..0x5A ('A'..'Z') gets 0x20 or-ed in,
 * every other byte is copied unchanged -- bytes >= 0x80 never change, so UTF-8 passes through whole and there is no
 * Latin-1 folding.  dst == src folds in place; neither pointer needs any alignment; n == 0 does nothing.
 * The _nocase builders fold the PATTERNS after they are read and before they are sorted: for the escaped reader after
 * escape decoding ("\x41" folds, the 'x' of an escape is never touched); in a class the listed set is folded (upper-case
 * members become their lower-case letters) and "[^...]" complements the folded set, so "[^A]" rejects 'a' -- and hence 'A'
 * once the input is folded.  Sorting, "the last line wins" among duplicates ("Foo" and "foo" are duplicates) and the
 * partition cuts act on the folded bytes.  The result is, blob for blob, the table the plain builder makes from a
 * pattern file folded beforehand; pfac_table and the blob do not record it, and nothing about the table says "fold":
 * the caller sets the scan's mode with pfac_table_set_case_fold after the upload.
 *   _mem_nocase            part / n_parts as pfac_table_build_mem_part; 0, 1 = the whole file
 *   _file_nocase           escapes != 0: the reader of pfac_table_build_file_escaped, else that of pfac_table_build_file */
int pfac_fold_ascii(void *dst, const void *src, size_t n);
int pfac_table_build_mem_nocase(const void *patterns, size_t n_bytes, int width, int part, int n_parts, pfac_table **out,
                                char *err, size_t err_len);
int pfac_table_build_file_nocase(const char *pattern_file, int width, int escapes, pfac_table **out, char *err,
                                 size_t err_len);
int pfac_table_build_mem_charclass_nocase(const void *patterns, size_t n_bytes, int width, pfac_table **out,
                                          pfac_outputs **outputs, char *err, size_t err_len);
int pfac_table_build_file_charclass_nocase(const char *pattern_file, int width, pfac_table **out, pfac_outputs **outputs,
                                           char *err, size_t err_len);

/* The device lookup evaluated on the host (property tests; never used on the scan path). */
int32_t pfac_table_lookup(const pfac_table *t, int32_t state, int32_t ch);
/* len[s] for s in [0, num_final): bytes of the pattern(s) ending in final state s (= its depth in the trie / DFA);
 * -1 for a final state no input reaches (a duplicate line's own state).  n must be >= num_final.  Computed from the
 * table alone (any source: files, _part, charclass, from_blob, from_reference_arrays) in O(n_keys + state_num). */
int pfac_table_final_lengths(const pfac_table *t, int32_t *len, size_t n);

/* Flat int32 image of a table: what gets uploaded, and what RCCL broadcasts
 * between ranks.  Layout: 16-word header {magic, version, width, width_bit,
 * n_patterns, num_final, state_num, max_pat_len, max_row, ht_size, n_keys,
 * 0...} then s0[256], r[max_row], HT[ht_size], val[ht_size], idmap[num_final]. */
#define PFAC_BLOB_MAGIC 0x50464143 /* "PFAC" */
#define PFAC_BLOB_VERSION 1
#define PFAC_BLOB_HEADER_WORDS 16
size_t pfac_table_blob_words(const pfac_table *t);
int pfac_table_to_blob(const pfac_table *t, int32_t *blob, size_t n_words);
int pfac_table_from_blob(const int32_t *blob, size_t n_words, pfac_table **out);
/* Wrap arrays produced by the reference's own FFDM() (main.cc:72-76,125) so a
 * reference build can feed this library without rebuilding its tables. */
int pfac_table_from_reference_arrays(const int32_t *s0, const int32_t *r, const int32_t *HT, const int32_t *val,
                                     const int32_t *idmap, int32_t width, int32_t state_num, int32_t num_final,
                                     int32_t ht_size, int32_t max_pat_len, pfac_table **out);

/* Text emitter: replaces main.cc:335-350.  One line per record,
 * "At position %4d, match pattern %d\n" with pos = base + rec.pos and
 * pattern = idmap[rec.state].  Appends to an open FILE* (void* to keep stdio
 * out of the ABI); returns bytes written (>= 0) or a negative status. */
typedef struct pfac_record {
    uint32_t pos;       /* start offset, relative to the first byte of the scanned range */
    uint32_t state;     /* final state reached (== index into idmap) */
} pfac_record;
/*
 * On the DEVICE the scan writes the COMPACT form of the same list: one word per match,  (pos & 4095) | state << 12,
 * as wide as the automaton needs -- 16 bits for at most 16 final states, 32 bits up to 2^20, else an 8-byte
 * pfac_record (pfac_scan_format tells which) -- into a record HEAP, plus an ordered TILE INDEX: the records of 4 KiB
 * input tile t are the PFAC_TIX_COUNT(tile_index[t]) words that start at word PFAC_TIX_FIRST(tile_index[t]), in
 * (position, pattern length) order, with  pos = t * 4096 + (word & 4095).  Walking the index in tile order yields the
 * reference's output order; the heap itself has small gaps and no global order (a workgroup fills chunks of it with
 * the tiles it scans -- a globally contiguous array would cost a chip-wide prefix over batches that are still being
 * scanned).  pfac_records_d2h / pfac_records_expand deliver ONE sorted pfac_record array whatever the form.
 */
#define PFAC_TILE_BYTES 4096
#define PFAC_PACKED_POS(word) ((uint32_t)(word) & 4095u)
#define PFAC_PACKED_STATE(word) ((uint32_t)(word) >> 12)
#define PFAC_TIX_FIRST(e) ((uint64_t)(e) & ((1ull << 40) - 1))
#define PFAC_TIX_COUNT(e) ((uint32_t)((uint64_t)(e) >> 40))
/* idmap == NULL: rec.state already holds the pattern id (the output of pfac_merge_partitions). */
int64_t pfac_emit_records(void *file, const pfac_record *rec, uint64_t n, uint64_t base, const int32_t *idmap);
/* Character-class tables: one line per (record, pattern ending in the record's final state), ascending pattern id. */
int64_t pfac_emit_records_multi(void *file, const pfac_record *rec, uint64_t n, uint64_t base, const pfac_outputs *outputs);
/* Same bytes, produced by n_threads host threads (size pass, prefix sum, format + pwrite in place); the serial
 * fprintf loop is the end-to-end wall once the scan runs at TB/s.  The file must be seekable; falls back to the
 * serial emitter for small n, n_threads < 2 or pipes. */
int64_t pfac_emit_records_mt(void *file, const pfac_record *rec, uint64_t n, uint64_t base, const int32_t *idmap,
                             int n_threads);
/* The same text straight from the compact device form (record heap + tile index as pfac_records_d2h_packed
 * delivers them), tiles in order: position = base + t * 4096 + PFAC_PACKED_POS(word), pattern =
 * idmap[PFAC_PACKED_STATE(word)]; record_bytes = 2 or 4 and n_words = heap words held by `words` (*used), as
 * pfac_scan_format reports.  A tile whose records would lie outside words[0, n_words) -> PFAC_E_ARG, nothing written.
 * n_threads < 2: serial. */
int64_t pfac_emit_packed(void *file, const void *words, uint64_t n_words, int record_bytes, const uint64_t *tile_index,
                         uint64_t n_tiles, uint64_t base, const int32_t *idmap, int n_threads);
/* Merge of per-partition match lists, replaces main.cc:304-324.  lists[k] (counts[k] records, sorted by
 * position as the scan emits them) comes from partition k of pfac_table_build_file_part(); the result is
 * ordered by (position, partition) -- i.e. by (position, pattern length), the reference's output order -- and
 * its `state` field holds the PATTERN ID: idmaps[k][state] (idmaps == NULL or idmaps[k] == NULL: the list
 * already holds ids).  Returns the number of records written, PFAC_E_OVERFLOW if out_cap is too small. */
int64_t pfac_merge_partitions(const pfac_record *const *lists, const uint64_t *counts, const int32_t *const *idmaps,
                              int n_parts, pfac_record *out, uint64_t out_cap);

/* ------------------------------------------------------------------ */
/* Device side (libpfac_hip.so): the master_kernel.cu path.            */

typedef struct pfac_ctx pfac_ctx;   /* one per GPU; holds what d_input_string/d_r/d_hash_table/
                                       d_match_result/d_val_table/d_s0Table held (main.cc:99-104) */

int pfac_device_count(int *n);                                       /* cudaGetDeviceCount, main.cc:50 */
/* Replaces cudaSetDevice + cudaStreamCreate (main.cc:183,209) and the
 * allocation half of GPU_Malloc_Memory (master_kernel.cu:188-257).
 * n_streams >= 1 independent pipeline slots ("streams per GPU", argv[2]). */
int pfac_ctx_create(int device, int n_streams, pfac_ctx **out);
void pfac_ctx_destroy(pfac_ctx *ctx);                                /* GPU_Free_memory, master_kernel.cu:457-524 */
const char *pfac_last_error(const pfac_ctx *ctx);                    /* ctx may be NULL: last error of the calling thread */

/* Table upload: the H2D copies of r/HT/s0/val and the texture binds
 * (master_kernel.cu:302-320,365-383).  blob is a pfac_table_to_blob image in
 * host memory; the _device variant takes an image already in this GPU's
 * memory (e.g. the receive buffer of an RCCL broadcast) and uses `stream_handle`
 * (a hipStream_t, may be NULL) for ordering. */
/* An upload waits for the scans still pending on the context's slots (they read the old tables); such a scan is
 * finished with pfac_scan_finish as usual.  The records of a scan made with an EARLIER table stay valid as records:
 * pfac_records_d2h, pfac_records_expand and the packed fetches deliver them, their `state` indexing the idmap of the
 * table they were scanned with.  Everything that needs that table on the device is gone with it: the text emitter and
 * the checksum (idmap), the segment pass, both selections and both replaces (final lengths, replacements) return
 * PFAC_E_STATE for such a scan.
 * An upload installs its table whole or not at all.  An image whose HEADER is refused (magic, version, sizes: PFAC_E_ARG)
 * leaves the installed table, what is attached to it and every earlier scan exactly as they were.  Any refusal past the
 * header -- an image whose states or displacements point outside its tables, a failed device allocation -- leaves the
 * context with NO table: pfac_scan_async, pfac_scan_info and the pfac_table_set_* calls return PFAC_E_STATE until an
 * upload succeeds, and every earlier scan counts as one made with an earlier table, as above. */
int pfac_table_upload(pfac_ctx *ctx, const int32_t *blob, size_t n_words);
int pfac_table_upload_device(pfac_ctx *ctx, const void *d_blob, size_t n_words, void *stream_handle);

/* Case-insensitive scans: the scan folds the INPUT on its way into the kernel's on-chip copy, with the fold of
 * pfac_fold_ascii -- bytes 0x41..0x5A get 0x20 or-ed in, no other byte changes (none >= 0x80: UTF-8 is safe).  The caller's
 * input buffer is never written.  Records, counts, the leftmost-longest selections and the emitted text are those of an
 * EXACT scan of the folded input with the same table; with a table from a _nocase builder (folded patterns) that is
 * grep -i.  With a table that holds upper-case letters the folded scan simply never takes those edges.
 * Every pass behind the scan that reads the input reads the ORIGINAL bytes: the whole-word filter judges them, both
 * replaces and the gather copy them (grep -i prints the line as it was written), the split cuts them.  A custom word set
 * that separates the cases therefore sees the case the input was written in.
 *   mode   PFAC_FOLD_NONE or PFAC_FOLD_ASCII; anything else: PFAC_E_ARG, and the setting stays as it was
 * PFAC_E_STATE before a table upload (as pfac_table_set_final_lengths).  The setting belongs to the uploaded table: it
 * holds until the next pfac_table_upload / pfac_table_upload_device, which resets it to PFAC_FOLD_NONE.  It applies to
 * every pfac_scan_async queued after the call, on every slot; a scan queued before keeps the mode it was launched with
 * (the mode is fixed at launch: every scan kernel has a twin that folds, and the launch picks one), so the call waits
 * for nothing and costs no device work.  An exact scan runs the kernel it always ran. */
#define PFAC_FOLD_NONE  0u
#define PFAC_FOLD_ASCII 1u
int pfac_table_set_case_fold(pfac_ctx *ctx, uint32_t mode);
/* The current setting (PFAC_FOLD_NONE after an upload).  PFAC_E_STATE before a table upload. */
int pfac_table_case_fold(pfac_ctx *ctx, uint32_t *mode);

/* Pinned host memory, replaces cudaHostAlloc(..., cudaHostAllocPortable) (main.cc:147,161). */
int pfac_host_alloc(void **p, size_t n_bytes);
void pfac_host_free(void *p);
/* Make an existing, page-aligned host range DMA-able in place -- e.g. a MAP_SHARED mapping of the input file: the H2D
 * copy then reads the page cache itself, and no CPU thread copies the input at all (gphf's default ingest).  Ranges
 * must not overlap; unregister before unmapping.  Fails (PFAC_E_HIP) where the driver cannot pin the pages. */
int pfac_host_register(void *p, size_t n_bytes);
int pfac_host_unregister(void *p);

/* Per-slot device buffers owned by the context.  Input capacity is rounded up
 * so the kernel's tile loads stay in bounds (master_kernel.cu:217 pads by
 * one tile + 512 B for the same reason), by less than two tiles.  Buffers only grow.  A request no larger than an
 * earlier one changes nothing.  A request that outgrows a buffer the slot already has REPLACES it, and the contents are
 * not kept: the call first waits for everything the slot still does with the old buffer (a pending scan, H2D copies),
 * and the slot then has NO FINISHED SCAN -- pfac_scan_finish, the record fetches, the text emitter, the checksum and
 * every pass return PFAC_E_STATE until the next pfac_scan_async, whichever buffers the lost scan used.  (Copying a
 * heap of up to gigabytes that its only callers -- the overflow retry, the next chunk -- are about to overwrite would
 * be wasted work; a caller that wants the old records fetches them first.)  Results of earlier passes in their own
 * slot-owned buffers (selection, segment, replace output, text) stay fetchable. */
int pfac_slot_reserve(pfac_ctx *ctx, int slot, uint64_t input_bytes, uint64_t record_capacity);
void *pfac_slot_input(pfac_ctx *ctx, int slot);          /* device pointer, 256-B aligned */
void *pfac_slot_records(pfac_ctx *ctx, int slot);        /* device pointer (record_capacity x 8 bytes, either record form) */
void *pfac_slot_stream(pfac_ctx *ctx, int slot);         /* the slot's hipStream_t */
/* Use an EXTERNAL stream (e.g. torch's current stream) for a slot; NULL restores the slot's own.  A change of stream
 * waits for everything the slot has queued on the old one (a scan, the asynchronous writes of a pass): what follows on
 * the new stream may read it. */
int pfac_slot_set_stream(pfac_ctx *ctx, int slot, void *stream_handle);

/* Async H2D of input bytes into the slot's input buffer at dst_offset
 * (cudaMemcpy H2D, master_kernel.cu:359, made asynchronous).  Ordered like a copy on the slot's stream: it starts
 * behind EVERYTHING the slot's stream has queued when the call is made, and what the slot queues afterwards starts behind
 * it.  That covers every reader of the slot's input, not the last scan alone: pfac_replace_leftmost_longest,
 * pfac_replace_documents, pfac_slot_doc_offsets_split and pfac_documents_gather return as soon as their size is known
 * and read the input once more from a kernel queued behind that, so the next chunk may be uploaded into the same slot
 * before their output has been fetched.  (The copies of all slots run on one copy stream of the context, in call order.)
 * Bytes written by other means -- a kernel of the caller's on another stream -- are the caller's to order. */
int pfac_slot_h2d(pfac_ctx *ctx, int slot, const void *host, uint64_t n_bytes, uint64_t dst_offset);
/* Block until the slot's last pfac_slot_h2d has left the host buffer (which may then be refilled while the scan that
 * follows it on the stream is still running): what lets a reader pool run ahead of the copies. */
int pfac_slot_h2d_wait(pfac_ctx *ctx, int slot);
/* The same question without blocking: 1 = it has, 0 = not yet, negative = error. */
int pfac_slot_h2d_done(pfac_ctx *ctx, int slot);

/*
 * The scan: replaces the kernel launch of GPU_TraceTable (master_kernel.cu:396-423).
 *   d_input   device pointer, 16-B aligned; NULL = the slot's own input buffer
 *   n_owned   start offsets [0, n_owned) are matched and reported   (<= 2^32)
 *   n_avail   bytes readable from d_input, n_owned <= n_avail; walks that
 *             start in the owned range may read up to n_avail (the halo of
 *             max_pat_len-1 bytes that belongs to the next shard) and never beyond
 *   d_records device pointer for the record heap, 16-B aligned, NULL = the slot's;
 *             at most capacity x 8 bytes are written (capacity x 2 or x 4 in the compact forms)
 *   capacity  records the heap holds.  It needs some slack over the match count (chunks a workgroup has not
 *             filled: at most capacity/16, plus gaps below 1 %); the match count is exact even when the
 *             heap overflows, and pfac_scan_capacity_hint() then says what to reserve
 * Through the tile index (which lives in the slot) the records are ordered by (pos, pattern length) == the
 * reference's output order (main.cc:341-349).  Asynchronous on the slot's stream.
 */
int pfac_scan_async(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_owned, uint64_t n_avail,
                    void *d_records, uint64_t capacity);
/* Wait for the slot and fetch the exact number of matches.  Returns
 * PFAC_E_OVERFLOW (with *n_matches set) when capacity was exceeded. */
int pfac_scan_finish(pfac_ctx *ctx, int slot, uint64_t *n_matches);
/* After pfac_scan_finish: a record capacity that the same scan fits (the finished scan's heap use + margin). */
int pfac_scan_capacity_hint(pfac_ctx *ctx, int slot, uint64_t *capacity);
/* Kernel time of the slot's last scan (the analogue of "2. MASTER: The elapsed
 * time is %f ms", master_kernel.cu:400-421): first workgroup in -> last
 * workgroup out, taken by the kernel itself from the device's constant-rate
 * clock.  The dispatch carries no events for it and pays nothing for it; the
 * figure leaves out the dispatch's ramp and the fence at its end, which an
 * event pair around the launch includes.  0 for an empty scan.  Waits for the
 * scan if it is still running. */
int pfac_scan_elapsed_ms(pfac_ctx *ctx, int slot, float *ms);
/* D2H of records [first, first+n) of the sorted sequence as pfac_record (the compact replacement of the dense
 * cudaMemcpy D2H, master_kernel.cu:428).  Asynchronous; pfac_slot_sync() completes it.  n == 0 does nothing.
 * PFAC_E_STATE without a scan or before its pfac_scan_finish, PFAC_E_OVERFLOW if the scan overflowed its heap,
 * PFAC_E_ARG when first + n exceeds the match count (same for pfac_records_expand). */
int pfac_records_d2h(pfac_ctx *ctx, int slot, const void *d_records, pfac_record *host, uint64_t first, uint64_t n);
int pfac_slot_sync(pfac_ctx *ctx, int slot);
/* Record form of the slot's last finished scan: *record_bytes = 2 or 4 (compact words) or 8 (pfac_record in the
 * heap); *n_tiles = tiles scanned = entries of the tile index; *used = heap records in use (<= capacity unless it
 * overflowed). */
int pfac_scan_format(pfac_ctx *ctx, int slot, int *record_bytes, uint64_t *n_tiles, uint64_t *used);
/* Records [first, first+n) of the slot's last scan, SORTED, as pfac_record in DEVICE memory (d_out, 8-B aligned), on
 * the slot's stream -- for consumers that stay on the GPU (the RCCL record gather). */
int pfac_records_expand(pfac_ctx *ctx, int slot, const void *d_records, uint64_t first, uint64_t n, pfac_record *d_out);
/* D2H of the compact form itself: heap words [0, n_words) (n_words = *used of pfac_scan_format; record_bytes each)
 * and the n_tiles entries of the tile index (2 or 4 bytes per match over PCIe instead of 8; pfac_emit_packed() prints
 * from it).  PFAC_E_STATE when the last scan was not compact. */
int pfac_records_d2h_packed(pfac_ctx *ctx, int slot, const void *d_records, void *host_words, uint64_t n_words,
                            uint64_t *host_tile_index);

/* GPU-side text emitter -- the fprintf loop of main.cc:335-350 run on the device: the records of the slot's last finished
 * scan -> the lines "At position %4d, match pattern %d\n" (position = base + pos, pattern = idmap[state] of the uploaded
 * table), in the reference's output order, into a device buffer the slot owns; *n_bytes = their total size.  Line length
 * depends on the digit counts: one kernel sizes the lines per 64 tiles, a prefix sum places them, a third formats -- the
 * host only copies finished text (pfac_text_d2h, asynchronous on the slot's stream; pfac_slot_sync completes it) and
 * write()s it.  base + 2^32 must stay below 10^18.  Byte-identical to pfac_emit_records / pfac_emit_packed.
 * (Character-class tables, whose final states may stand for several patterns, print on the host: pfac_emit_records_multi;
 * the device prints idmap[state], the first id, once.)  PFAC_E_STATE without a finished scan or for a scan made with an
 * earlier table, PFAC_E_OVERFLOW if the scan overflowed its heap. */
int pfac_emit_text_device(pfac_ctx *ctx, int slot, const void *d_records, uint64_t base, uint64_t *n_bytes);
int pfac_text_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n_bytes);
void *pfac_slot_text(pfac_ctx *ctx, int slot);            /* device pointer of that text (valid until the slot's next pfac_emit_text_device) */

/* The compact form handed to a consumer that STAYS ON THE DEVICE (the RCCL record gather sends it: 2 or 4 bytes per
 * match plus 8 bytes per 4 KiB tile over xGMI instead of 8-byte pfac_records): the n_tiles entries of the slot's tile
 * index -> d_tile_index_out and, unless d_words_out is NULL or the record heap itself, heap words [0, n_words) ->
 * d_words_out (device pointers; n_words = *used of pfac_scan_format).  Asynchronous on the slot's stream. */
int pfac_records_packed_device(pfac_ctx *ctx, int slot, const void *d_records, void *d_words_out, uint64_t n_words,
                               uint64_t *d_tile_index_out);

/* Order-independent 64-bit checksum of ALL records of the slot's last scan (sum over records of
 * mix(base+pos, idmap[state])), computed on the GPU; used for full-size parity checks where materialising
 * the text is not practical.  n = the scan's match count (0: checksum of nothing).  For n > 0: PFAC_E_STATE without a
 * finished scan or for a scan made with an earlier table, PFAC_E_OVERFLOW if the scan overflowed its heap. */
int pfac_records_checksum(pfac_ctx *ctx, int slot, const void *d_records, uint64_t n, uint64_t base,
                          uint64_t *checksum);

/* How often did each pattern match?  The histogram of the FINAL STATES of the slot's last finished scan, computed on the
 * GPU from the record heap and the tile index (the bytes the checksum reads; no input byte is read):
 *   counts[s] (+)= number of records whose final state is s,  0 <= s < n_states.
 * The heap is read through the tile index, so after pfac_records_filter_words the kept records are what is counted.
 * *n_counted = the scan's current match count = the sum of the counts added.  The host turns states into pattern ids
 * (idmap[s]; for character-class tables every id of outputs->ids[first[s] .. first[s+1])).
 *   d_records  NULL = the slot's heap; else the heap the scan wrote (any other pointer: PFAC_E_ARG)
 *   d_counts   NULL = a slot-owned buffer (fetched with pfac_state_counts_d2h); else a device pointer, 8-B aligned, of
 *              n_states entries: exactly n_states x 8 bytes are written and none beyond
 *   n_states   must equal num_final of the uploaded table (else PFAC_E_ARG); the kernel never writes a counter at or
 *              past n_states whatever the records hold
 *   flags      0: the counts are zeroed first.  PFAC_COUNT_ACCUMULATE: the call adds -- on a caller's buffer onto
 *              whatever is there; on the slot-owned buffer onto the counts the slot holds (from zero if it holds none),
 *              PFAC_E_STATE if those belong to an earlier table.  Chained ranges (owned ranges with the usual
 *              max_pat_len - 1 halo) and chunked streams are thereby exact on the device: the counts accumulated over the
 *              ranges are the counts of one scan of the whole.
 * Both calls are read-only on the heap, the tile index, the match count, the selection and every other pass's slot-owned
 * result.  The two share the slot-owned counts and are one pass; the counts stay fetchable, unchanged, through scans,
 * table uploads, pfac_slot_reserve and every other pass (the lifetime rule of pfac_segment_d2h) until the slot's next
 * count into the slot-owned buffer SUCCEEDS (which accumulation needs): a call that fails, or counts into a caller's
 * buffer, leaves them as they were.
 * Returns once *n_counted is known, like the checksum; the counts are then complete on the slot's stream.
 * PFAC_E_STATE: no finished scan (also after a pfac_slot_reserve that dropped it), a scan made with an earlier table.
 * PFAC_E_OVERFLOW: the scan overflowed its heap.  PFAC_E_ARG: flags outside 0..1, a wrong n_states, a misaligned d_counts,
 * a d_records that is not this scan's heap.  The scan's state is judged before the arguments (PFAC_E_STATE, then
 * PFAC_E_OVERFLOW, then the rest), as in pfac_records_filter_words.  Every error leaves the counts, slot-owned or caller's,
 * as they were.
 * Kernel: one wave per tile at a time, as the checksum; a workgroup keeps 32-bit partial counts in LDS -- a table indexed
 * by state up to 8192 final states (32 KiB), above that a direct-mapped cache of 16384 {state, count} slots (128 KiB, one
 * workgroup per CU) that a state claims on first sight (a state that finds its slot taken adds to memory at once) -- and
 * adds the non-zero ones to the 64-bit counters once, with agent-scope atomics.  Where one state fills a good part of a
 * chunk of 64 records (a wave probes for that every 16th chunk) the chunk is pre-aggregated by ballot, so that the one hot
 * state of a small pattern set costs one LDS add per chunk instead of 64 serialised ones. */
#define PFAC_COUNT_ACCUMULATE 1u   /* add onto the counts already there instead of zeroing them first */
int pfac_records_count_states(pfac_ctx *ctx, int slot, const void *d_records, uint64_t *d_counts, uint64_t n_states,
                              uint32_t flags, uint64_t *n_counted);
/* The same over the slot's last leftmost-longest selection (whole-stream or per-document): counts[s] (+)= picks whose state
 * is s; *n_counted = the number of picks.  d_sel: NULL = the slot-owned selection, else the caller's d_out of that
 * selection -- the rule and the answers of pfac_replace_leftmost_longest's d_sel: PFAC_E_STATE without a selection since
 * the slot's last scan (a new scan or a whole-word filter makes it stale), for a selection made with an earlier table, or
 * for NULL when the selection went to the caller's buffer; PFAC_E_ARG for a misaligned d_sel or one that is not a selection
 * of this table (a state at or past n_states, positions that do not ascend: checked on the device before any counter
 * changes).  d_counts, n_states, flags and the errors' effect as above; the selection's state is judged before the arguments
 * (PFAC_E_STATE, then the rest), and among the arguments, and between them and the accumulate onto counts of an earlier
 * table, no order is promised -- in either call.  A selection call that failed, PFAC_E_OVERFLOW for a too-small caller's
 * d_out included, leaves no selection (passing the d_out of the one before does not bring it back).  New document offsets
 * for the slot do not make a per-document selection stale here: the picks are counted as they were written, only the
 * per-document replace cuts them again. */
int pfac_selection_count_states(pfac_ctx *ctx, int slot, const pfac_record *d_sel, uint64_t *d_counts, uint64_t n_states,
                                uint32_t flags, uint64_t *n_counted);
/* D2H of the slot-owned counts (n_states entries of the call that wrote them).  Asynchronous on the slot's stream;
 * pfac_slot_sync completes it.  PFAC_E_STATE when the slot holds no counts. */
int pfac_state_counts_d2h(pfac_ctx *ctx, int slot, uint64_t *host_counts);

/* Batches of documents.  One scan covers one contiguous byte range; a batch of independent documents is scanned as
 * their concatenation and then cut into documents on the device.  Records are keyed by their START offset and a walk
 * is failureless, so the matches of document [a, b) are exactly the records of the concatenated scan with
 * a <= pos < b and pos + len(pattern) <= b: the cut drops the records that run across a document end, rebases the
 * others to their document and builds a per-document index.  The scan itself is unchanged.
 *
 * Final-state lengths for the uploaded table (host array, n == num_final, values -1 or 1..1024; see
 * pfac_table_final_lengths); kept on the device (16-bit) until the next pfac_table_upload / pfac_table_upload_device,
 * which clears them. */
int pfac_table_set_final_lengths(pfac_ctx *ctx, const int32_t *len, size_t n);
/* Document boundaries for a slot: n_docs + 1 offsets, copied into a slot-owned device buffer on the slot's stream
 * (the host array may be reused when the call returns). */
int pfac_slot_doc_offsets(pfac_ctx *ctx, int slot, const uint64_t *host_offsets, uint64_t n_docs);
/* Document boundaries from a delimiter byte, made ON THE DEVICE from bytes that are already there (a log or a JSONL
 * stream cut at '\n'): no host pass over the input, no upload of 8 bytes per line.  A document ends AFTER every delimiter
 * byte:
 *   E        = { i + 1 : 0 <= i < n_bytes, in[i] == delimiter }, ascending
 *   offsets  = 0, then E, then n_bytes once more if n_bytes > 0 and in[n_bytes - 1] != delimiter
 *   *n_docs  = number of offsets - 1;  n_bytes == 0: the single offset 0, *n_docs == 0
 *   *tail_start = the start of the unterminated last document, or n_bytes if there is none: a chunked reader carries
 *              in[tail_start : n_bytes] over to the next chunk.
 * A run of delimiters yields documents that hold only their delimiter.  A document keeps its trailing delimiter, so a
 * pattern that ends in '\n' (escaped pattern files) still matches inside its line.  The offsets satisfy the rules of
 * pfac_records_segment by construction (off[0] == 0, non-decreasing, off[n_docs] == n_bytes).
 *   d_input    NULL = the slot's input buffer (PFAC_E_ARG if n_bytes exceeds it); else a device pointer, 16-B aligned
 *   n_bytes    <= 2^32
 *   delimiter  0..255, else PFAC_E_ARG
 * No byte at or past n_bytes influences the result, whatever the buffer holds there: whole 16-byte chunks inside
 * [0, n_bytes) are loaded as such, the last partial one byte by byte.
 * Effect: exactly that of a successful pfac_slot_doc_offsets with the same offsets -- they live in the slot-owned buffer,
 * every document pass takes them with d_doc_offsets = NULL and *n_docs, and a per-document selection made before is
 * refused by pfac_replace_documents(d_doc_offsets = NULL).  The call needs no finished scan and reads no scan state; it
 * runs on the slot's stream, behind the slot's H2D copies, before or after the scan of the same bytes.  It returns once
 * *n_docs and *tail_start are known (one 16-byte copy back, which also sizes the buffer); the offsets are then written
 * asynchronously on the slot's stream.  PFAC_E_ARG also for a misaligned d_input, n_bytes > 2^32, and a result of 2^32
 * documents (every one of 2^32 bytes a delimiter).  Every error leaves the slot's offsets as they were.
 * Kernels: delimiters per 4 KiB tile (one wave per tile at a time, four dwordx4 loads per lane, an exact SWAR byte
 * compare), sums per group of 64 tiles, the group prefix, then the same loads again and one store of i + 1 per delimiter
 * at 1 + its rank; a tile without a delimiter is not read a second time. */
int pfac_slot_doc_offsets_split(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, int delimiter,
                                uint64_t *n_docs, uint64_t *tail_start);
/* D2H of offsets [first, first + n) of the slot's document offsets, whichever call set them.  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it.  PFAC_E_STATE if the slot holds none, PFAC_E_ARG when first + n exceeds
 * n_docs + 1. */
int pfac_slot_doc_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_offsets, uint64_t first, uint64_t n);
/* The slot's last finished scan, cut into documents [off[d], off[d+1]):
 *   d_records      the scan's record heap, NULL = the slot's
 *   d_doc_offsets  device uint64[n_docs + 1], NULL = the slot's (pfac_slot_doc_offsets, same n_docs).  Required:
 *                  off[0] == 0, non-decreasing, off[n_docs] == the scan's n_owned; empty documents allowed;
 *                  n_docs < 2^32.
 *   keeps a record (pos, state) of document d iff pos + len[state] <= off[d+1]; writes it as {pos - off[d], state}
 *   to d_out[k] in scan order (= (document, offset, pattern length) order), and d_doc_first[d] = index of document d's
 *   first kept record, d_doc_first[n_docs] = *n_kept.
 *   d_out / d_doc_first NULL = slot-owned buffers grown to fit (fetched with pfac_segment_d2h); else device pointers,
 *   8-B aligned, d_out holding out_cap records and d_doc_first n_docs + 1 entries.
 * Returns once *n_kept is known; the writes are asynchronous on the slot's stream (pfac_slot_sync completes them).
 * PFAC_E_OVERFLOW (with *n_kept exact, nothing written) when out_cap is too small for a caller's d_out;
 * PFAC_E_ARG for offsets that break the rules above (checked on the device, nothing written);
 * PFAC_E_STATE without a finished scan, for a scan made with an earlier table, or without lengths for the current
 * table; PFAC_E_OVERFLOW if the scan overflowed.
 * Three kernels: kept records per tile and per group of 64 tiles (the offsets are checked in the same pass), the
 * prefix over the groups, and the write; they read the record heap, the tile index, the offsets and the lengths,
 * never the input bytes. */
int pfac_records_segment(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                         pfac_record *d_out, uint64_t out_cap, uint64_t *d_doc_first, uint64_t *n_kept);
/* D2H of the slot-owned result of the last pfac_records_segment (host_records: *n_kept records, may be NULL when
 * d_out was the caller's; host_doc_first: n_docs + 1 entries, may be NULL when d_doc_first was the caller's).
 * Asynchronous on the slot's stream; pfac_slot_sync completes it.
 * Lifetime of a pass's slot-owned result (the same for the selections, the replaces and their fetches below): it stays
 * fetchable, unchanged, until the slot's next call of the SAME pass -- through later scans, table uploads, other passes,
 * pfac_slot_reserve, pfac_slot_doc_offsets and pfac_table_set_replacements (a replace output holds the bytes of the
 * replacements set when it ran).  The next call of the same pass discards it even when that call fails; the fetch then
 * returns PFAC_E_STATE, as it does when the pass wrote into the caller's buffers.  The two selections share one
 * slot-owned buffer and count as one pass here; so do the two replaces.  The extraction
 * (pfac_extract_leftmost_longest) is a pass of its own: neither it nor a replace discards the other's result. */
int pfac_segment_d2h(pfac_ctx *ctx, int slot, pfac_record *host_records, uint64_t *host_doc_first);

/* Which documents matched?  (grep -F -f patterns over lines; PFAC_DOCS_INVERT: grep -v.)  Document d is reported iff
 *   (doc_first[d + 1] > doc_first[d]) != invert;
 * the ids are written ascending, *n_matching of them.  doc_first[d + 1] - doc_first[d] is document d's match count, so
 * grep -c needs no call of its own: it is the difference of two fetched entries.
 *   d_doc_first  NULL = the slot-owned doc_first of the slot's last pfac_records_segment (PFAC_E_STATE if there is none
 *                or it went to the caller's buffer, PFAC_E_ARG if n_docs differs from that call's); else any device
 *                array of n_docs + 1 entries, 8-B aligned -- the caller's d_doc_first of the segment pass or of
 *                pfac_records_leftmost_longest_documents: a document has a pick iff it has a kept record, so either
 *                gives the same ids
 *   d_ids_out    NULL = a slot-owned buffer grown to fit (fetched with pfac_documents_matching_d2h; the lifetime rule of
 *                pfac_segment_d2h); else 8-B aligned, out_cap entries.  No entry at or past *n_matching is written.
 *   n_docs       < 2^32; 0 gives 0 ids
 * It reads nothing but doc_first.  Returns once *n_matching is known; the writes are asynchronous on the slot's stream.
 * PFAC_E_OVERFLOW (with *n_matching exact, nothing written) when out_cap is too small for a caller's d_ids_out;
 * PFAC_E_ARG for flags outside 0..1 or misaligned buffers.
 * Kernels: an ordered stream compaction -- one wave per 64 blocks of 64 documents, ballot and popcount per block, the
 * group prefix, then the write at group prefix + blocks before + ballot rank. */
#define PFAC_DOCS_INVERT 1u   /* the documents WITHOUT a kept record (grep -v) */
int pfac_documents_matching(pfac_ctx *ctx, int slot, const uint64_t *d_doc_first, uint64_t n_docs, uint32_t flags,
                            uint64_t *d_ids_out, uint64_t out_cap, uint64_t *n_matching);
/* D2H of the slot-owned ids of the last pfac_documents_matching (*n_matching entries).  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it. */
int pfac_documents_matching_d2h(pfac_ctx *ctx, int slot, uint64_t *host_ids);
/* pfac_documents_matching with context lines (grep -B before, -A after; -C n is both).  Document d is reported iff some
 * document e with d - after <= e <= d + before has a kept record, both window ends clamped to [0, n_docs - 1]:
 *   doc_first[min(d + before, n_docs - 1) + 1] > doc_first[d - min(d, after)]
 * -- doc_first is a prefix array, so the question about a window costs the same two loads as the one about a document.
 * Any before / after up to 2^64 - 1 is legal and clamps (d + before does not wrap).  The ids are ascending and each
 * appears once: overlapping contexts merge, as in grep; grep's "--" separator lines are not produced.  With
 * before == after == 0 the result is that of pfac_documents_matching(flags = 0).
 *   flags   must be 0.  PFAC_DOCS_INVERT gives PFAC_E_ARG: context around the documents WITHOUT a record asks whether a
 *           window holds a document with no record, which needs the number of matching documents in the window; a
 *           prefix of record counts does not give it (one document with many records and many with one look alike).
 * d_doc_first, d_ids_out, out_cap, *n_matching, PFAC_E_OVERFLOW (exact count, nothing written), the alignment and
 * n_docs < 2^32 are exactly those of pfac_documents_matching.  The two calls are ONE pass: they share the slot-owned id
 * buffer and pfac_documents_matching_d2h, and the next call of either discards the result, even when that call fails.
 * Kernels: the compaction of pfac_documents_matching, instantiated with the window flag. */
int pfac_documents_matching_context(pfac_ctx *ctx, int slot, const uint64_t *d_doc_first, uint64_t n_docs, uint64_t before,
                                    uint64_t after, uint32_t flags, uint64_t *d_ids_out, uint64_t out_cap, uint64_t *n_matching);

/* The selected documents' bytes, back to back in one device buffer (what grep prints; with the two calls above the line
 * path ends on the device like every other consumer).  With off = the document offsets and len(k) = off[ids[k] + 1] -
 * off[ids[k]]:
 *   out_off[k]     = sum of len(j) over j < k;  out_off[n_ids] = *out_bytes
 *   out[out_off[k] : out_off[k + 1]] = in[off[ids[k]] : off[ids[k] + 1]]
 *   d_input        NULL = the slot's input buffer (PFAC_E_ARG if n_bytes exceeds it); else a device pointer, 16-B aligned
 *   n_bytes        <= 2^32: the bytes readable.  No byte at or past n_bytes is read: whole 16-byte chunks inside
 *                  [0, n_bytes) are loaded as such, also where they reach outside a selected document, the last partial
 *                  one byte by byte (the rule of pfac_slot_doc_offsets_split)
 *   d_doc_offsets  NULL = the slot's offsets, whichever call set them (PFAC_E_STATE if there are none or n_docs is not
 *                  theirs, as in pfac_records_filter_words); else device uint64[n_docs + 1], 8-B aligned; n_docs < 2^32
 *   d_ids          NULL = the slot-owned ids of the slot's last pfac_documents_matching or _context (PFAC_E_STATE if there
 *                  are none or they went to the caller's buffer, PFAC_E_ARG if n_ids differs from that call's count);
 *                  else device uint64[n_ids], 8-B aligned, n_ids < 2^32.  The ids may come in ANY order and may repeat:
 *                  a caller may gather a permutation, or a document twice
 *   d_out          NULL = a slot-owned buffer grown to fit (fetched with pfac_documents_gather_d2h); else 16-B aligned,
 *                  out_cap bytes.  No byte at or past *out_bytes is written (only the last partial 16 B is stored in
 *                  pieces), so a buffer of exactly *out_bytes bytes is enough
 *   d_out_offsets  NULL = a slot-owned buffer (pfac_documents_gather_offsets_d2h); else 8-B aligned, n_ids + 1 entries
 * Checked on the device, in the first pass, before anything is written: every ids[k] < n_docs, and off[ids[k]] <=
 * off[ids[k] + 1] <= n_bytes -- for the SELECTED documents only (offsets that break the rule at a document nobody
 * selected do not matter).  A violation gives PFAC_E_ARG.
 * Returns once *out_bytes is known (one 16-byte copy back: the total and the error word); the offsets and the bytes are
 * then written asynchronously on the slot's stream (pfac_slot_sync completes them).  PFAC_E_OVERFLOW (with *out_bytes
 * exact) when out_cap is too small for a caller's d_out; PFAC_E_ARG also for misaligned buffers, n_bytes > 2^32, n_docs or
 * n_ids >= 2^32.  EVERY error leaves every caller's buffer of the call untouched, d_out_offsets included: the offsets
 * are written behind the host's check of the total.  n_ids == 0: *out_bytes = 0, out_off[0] = 0 is written, nothing else.
 * The call needs no finished scan and reads no scan state, like the split; it only reads the input, the offsets and the
 * ids.  The slot-owned result follows the lifetime rule of pfac_segment_d2h: the next pfac_documents_gather discards it
 * even when that call fails; the fetches then return PFAC_E_STATE, as they do when the output went to the caller's
 * buffers.
 * Kernels: lengths per block of 64 ids and per group of 1024 (two 8-byte gathers of the offsets per id, the checks in
 * the same pass), the group prefix, out_off per id, then an output-driven write in the shape of the replace's: every
 * wave owns windows of 1 KiB, finds the id that holds the window's first byte by a galloping search over the block
 * offsets (never a walk from id 0; 1-byte and empty documents are skipped by the block), each lane assembles its 16
 * bytes in registers from the unaligned source runs that cover it and stores one dwordx4. */
int pfac_documents_gather(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, const uint64_t *d_doc_offsets,
                          uint64_t n_docs, const uint64_t *d_ids, uint64_t n_ids, void *d_out, uint64_t out_cap,
                          uint64_t *d_out_offsets, uint64_t *out_bytes);
/* D2H of bytes [first, first + n) of the slot-owned output of the last pfac_documents_gather.  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it.  first + n > *out_bytes gives PFAC_E_ARG; n == 0 does nothing. */
int pfac_documents_gather_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n);
/* D2H of the slot-owned output offsets of the last pfac_documents_gather (n_ids + 1 entries).  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it. */
int pfac_documents_gather_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_out_offsets);

/* The gather with labels: the finished text of grep -n, -b, -A / -B / -C and the final newline.  Segment k of the output
 * is, in this order (id = ids[k], off = the document offsets):
 *   1. group_sep[0 : group_sep_len], if group_sep_len > 0 and either k > 0 && ids[k] != ids[k - 1] + 1 (a repeat or a
 *      descending step is "not adjacent"), or k == 0 with PFAC_LINE_SEP_FIRST
 *   2. with PFAC_LINE_NUMBER: the decimal of id + number_base, no padding, then the label separator
 *   3. with PFAC_LINE_OFFSET: the decimal of off[id] + offset_base, then the label separator
 *   4. the body, in[off[id] : off[id + 1]]
 *   5. with PFAC_LINE_TERMINATE: the byte `terminator`, if the document is empty or its last byte is not `terminator`
 * out_off[k] is the offset of segment k's first byte, its group separator included; out_off[n_ids] = *out_bytes.
 * The label separator is sep_match; under PFAC_LINE_CONTEXT_SEP it is sep_context where doc_first[id + 1] ==
 * doc_first[id] (a context line: a document without a kept record).  d_doc_first is read only under that flag: NULL =
 * the slot-owned doc_first of the slot's last pfac_records_segment, with the rules and errors of
 * pfac_documents_matching (PFAC_E_STATE if the slot holds none, PFAC_E_ARG if n_docs is not that call's).
 * A chunked reader continues the numbering with number_base and offset_base (the lines and bytes of the chunks before
 * this one) and PFAC_LINE_SEP_FIRST (the chunk before printed a line that the first one here does not follow).
 * fmt == NULL, or a fmt with flags == 0 and group_sep_len == 0, gives output and offsets byte for byte those of
 * pfac_documents_gather.  Every other argument follows pfac_documents_gather: its checks on the device before anything
 * is written, PFAC_E_OVERFLOW with *out_bytes exact and every caller's buffer untouched, n_ids == 0 writing the single
 * offset 0 (a separator stands in front of a segment, never on its own).  PFAC_E_ARG also for flags outside the five,
 * group_sep_len > 8, and number_base + n_docs > 10^18 or offset_base + n_bytes > 10^18 (every printed value has at most
 * 18 digits).  Input reads stay below n_bytes: the terminator test reads in[off[id + 1] - 1] and nothing else, whole
 * 16-byte loads follow the gather's rule.  No byte at or past *out_bytes is written.
 * The call is ONE pass with pfac_documents_gather: they share the slot-owned output and offsets,
 * pfac_documents_gather_d2h and pfac_documents_gather_offsets_d2h fetch either call's result, and the next call of
 * either discards it, even when that call fails.
 * Kernels: siblings of the gather's.  The count pass adds the label lengths (digit counts), the id in front (a lane
 * shuffle) and, under PFAC_LINE_TERMINATE, one input byte; the write keeps each segment's id, source offset and piece
 * lengths (one 32-bit word) in LDS and makes the digits a lane owns in registers -- one divide by a power of ten, then
 * peeled by 10 -- so the output is written once, in whole 16-byte stores, with no scratch copy of the labels. */
#define PFAC_LINE_NUMBER      1u   /* decimal of ids[k] + number_base, then the label separator          */
#define PFAC_LINE_OFFSET      2u   /* decimal of off[ids[k]] + offset_base, then the label separator     */
#define PFAC_LINE_TERMINATE   4u   /* append `terminator` to a document that is empty or does not end in it */
#define PFAC_LINE_CONTEXT_SEP 8u   /* label separator = sep_context for a document without a kept record */
#define PFAC_LINE_SEP_FIRST  16u   /* the group separator also in front of ids[0]                        */
#define PFAC_LINE_MAX_GROUP_SEP 8u
typedef struct pfac_line_format {
    uint32_t flags;
    uint8_t  sep_match;        /* ':' */
    uint8_t  sep_context;      /* '-' */
    uint8_t  terminator;       /* '\n' */
    uint8_t  group_sep_len;    /* 0..8; 0 = no group separators */
    uint8_t  group_sep[8];     /* "--\n" */
    uint64_t number_base;      /* grep -n: 1 */
    uint64_t offset_base;      /* bytes of the chunks before this one */
} pfac_line_format;
int pfac_documents_gather_format(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, const uint64_t *d_doc_offsets,
                                 uint64_t n_docs, const uint64_t *d_ids, uint64_t n_ids, const uint64_t *d_doc_first,
                                 const pfac_line_format *fmt, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                 uint64_t *out_bytes);

/* Pattern groups: which of the caller's pattern CLASSES occur in each document (content rules whose strings must all
 * occur, grep -e groups joined by AND / NOT, label sets per line).  masks[s] is a 64-bit set: bit g is set iff the
 * pattern(s) that end in final state s belong to group g, 0 <= g < 64.  A state with mask 0 belongs to no group; the
 * scan still matches it and every other pass still sees it.  n_states must be num_final of the uploaded table, else
 * PFAC_E_ARG and the earlier masks stay; PFAC_E_STATE before a table upload.  The masks live on the device with the
 * table, like the final lengths: the next pfac_table_upload / _upload_device clears them (a failed upload past the header
 * leaves none), a second call replaces them.  The call waits for no scan; a group pass already queued keeps the masks
 * it was launched with (the old buffer is freed behind it, as pfac_table_set_replacements frees its own).  More than 64
 * groups: set other masks and run the pass again. */
int pfac_table_set_state_groups(pfac_ctx *ctx, const uint64_t *masks, uint64_t n_states);
/* A group mask per document, straight from the record heap of the slot's last finished scan:
 *   mask[d] = OR of masks[state] over the records (pos, state) with off[d] <= pos and pos + len[state] <= off[d + 1]
 * -- the keep rule of pfac_records_segment: a record that runs across a document's end counts for no document.  A
 * document without such a record, an empty one included, gets 0.  After pfac_records_filter_words only the kept records
 * count; the records of a folded scan count as they are.  The heap is read through the tile index; no input byte is read.
 *   d_records      the scan's record heap, NULL = the slot's; anything else that is not that heap gives PFAC_E_ARG
 *   d_doc_offsets  device uint64[n_docs + 1] under the rules of pfac_records_segment (checked on the device, in the same
 *                  pass); NULL = the slot's offsets, whichever call set them, with the same n_docs, else PFAC_E_STATE
 *   d_masks_out    NULL = a slot-owned buffer grown to fit (fetched with pfac_group_masks_d2h; the lifetime rule of
 *                  pfac_segment_d2h); else a device pointer, 8-B aligned: exactly n_docs x 8 bytes are written
 *   *any_mask      the OR of all mask[d]: the groups that occurred at all
 * Returns once *any_mask and the offsets' flag are known (one 16-byte copy back); the masks are then complete on the
 * slot's stream (pfac_slot_sync).  Judged in this order -- PFAC_E_STATE: no finished scan, a scan made with an earlier
 * table, no final lengths or no state groups for the current table, no offsets for the slot; PFAC_E_OVERFLOW: the scan
 * overflowed its heap; PFAC_E_ARG: misaligned buffers, n_docs >= 2^32, a d_records that is not this scan's heap, offsets
 * that break the rules.  Every error leaves a caller's buffer as it was (the masks are made in the slot's buffer and
 * copied behind the host's check of the offsets' flag); the slot-owned result is discarded even when the call fails.
 * n_docs == 0 (then n_owned == 0) writes nothing and sets *any_mask = 0.
 * One kernel behind a memset of the masks: one wave per 64 tiles walks the records as the segment pass's count does,
 * ORs the masks of a document's records in registers (a segmented OR scan over the 64 lanes, the open run carried across
 * chunks and tiles) and writes each document once -- a plain 8-byte store where the document lies inside the wave's
 * tiles, an atomic OR for the at most two that straddle their ends.  No atomic per record. */
int pfac_documents_group_masks(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                               uint64_t *d_masks_out, uint64_t *any_mask);
/* D2H of masks [first, first + n) of the slot-owned result of the last pfac_documents_group_masks.  Asynchronous on the
 * slot's stream; pfac_slot_sync completes it.  first + n > n_docs gives PFAC_E_ARG; n == 0 does nothing. */
int pfac_group_masks_d2h(pfac_ctx *ctx, int slot, uint64_t *host_masks, uint64_t first, uint64_t n);
/* The documents whose group mask m = mask[d] satisfies a predicate.  Document d is reported iff
 *   ((m & all_of) == all_of && (any_of == 0 || (m & any_of) != 0) && (m & none_of) == 0) != invert
 * (flags: 0 or PFAC_DOCS_INVERT); all_of = none_of = 0, any_of = ~0 is "some grouped pattern matched".
 *   d_masks  NULL = the slot-owned masks of the slot's last pfac_documents_group_masks (PFAC_E_STATE if there are none or
 *            they went to the caller's buffer, PFAC_E_ARG if n_docs differs from that call's); else any device
 *            uint64[n_docs], 8-B aligned
 * d_ids_out, out_cap, *n_matching, PFAC_E_OVERFLOW (exact count, nothing written), the alignment and n_docs < 2^32 are
 * exactly those of pfac_documents_matching, and the call is ONE pass with it and _context: the same slot-owned id
 * buffer, pfac_documents_matching_d2h, and pfac_documents_gather(d_ids = NULL) consumes its ids unchanged.
 * Kernels: the compaction of pfac_documents_matching, instantiated with the predicate (one load per document). */
int pfac_documents_matching_groups(pfac_ctx *ctx, int slot, const uint64_t *d_masks, uint64_t n_docs, uint64_t all_of,
                                   uint64_t any_of, uint64_t none_of, uint32_t flags, uint64_t *d_ids_out, uint64_t out_cap,
                                   uint64_t *n_matching);

/* Document scores: HOW MUCH of the pattern set a document holds (a blocklist's hit count, hits per 1000 bytes, a rule
 * engine's weighted sum against a threshold, grep -c per document).  weights[s] is the weight of final state s, any
 * int32, 0 included.  n_states must be num_final of the uploaded table, else PFAC_E_ARG and the earlier weights stay;
 * PFAC_E_STATE before a table upload.  The weights live on the device with the table, like the state groups: the next
 * pfac_table_upload / _upload_device clears them, a second call replaces them.  The call waits for no scan; a score
 * pass already queued keeps the weights it was launched with (the old buffer is freed behind it). */
typedef struct {
    int64_t  score;            /* sum of the weights, two's-complement wrap */
    uint64_t count;            /* records summed */
} pfac_doc_score;              /* 16 bytes */
int pfac_table_set_state_weights(pfac_ctx *ctx, const int32_t *weights, uint64_t n_states);
/* A score per document, straight from the record heap of the slot's last finished scan: over the records (pos, state)
 * with off[d] <= pos and pos + len[state] <= off[d + 1] -- the keep rule of pfac_records_segment --
 *   count[d] = how many there are,   score[d] = the sum of weights[state], in int64 with two's-complement wrap.
 * A record of weight 0 counts.  A document without such a record, an empty one included, gets {0, 0}.  After
 * pfac_records_filter_words / _filter_spans only the kept records count; the records of a folded scan count as they
 * are.  The heap is read through the tile index; no input byte is read.
 *   d_records      the scan's record heap, NULL = the slot's; anything else that is not that heap gives PFAC_E_ARG
 *   d_doc_offsets  device uint64[n_docs + 1] under the rules of pfac_records_segment (checked on the device, in the same
 *                  pass); NULL = the slot's offsets, whichever call set them, with the same n_docs, else PFAC_E_STATE
 *   d_scores_out   NULL = a slot-owned buffer grown to fit (fetched with pfac_document_scores_d2h; the lifetime rule of
 *                  pfac_segment_d2h); else a device pointer, 16-B aligned: exactly n_docs x 16 bytes are written
 *   *total         the sums of score[d] and count[d] over all documents
 * Returns once *total and the offsets' flag are known (one 24-byte copy back); the scores are then complete on the
 * slot's stream (pfac_slot_sync).  Judged in this order -- PFAC_E_STATE: no finished scan, a scan made with an earlier
 * table, no final lengths or no state weights for the current table, no offsets for the slot; PFAC_E_OVERFLOW: the scan
 * overflowed its heap; PFAC_E_ARG: misaligned buffers, n_docs >= 2^32, a d_records that is not this scan's heap, offsets
 * that break the rules.  Every error leaves a caller's buffer as it was (the scores are made in the slot's buffer and
 * copied behind the host's check of the offsets' flag); the slot-owned result is discarded even when the call fails.
 * n_docs == 0 (then n_owned == 0) writes nothing and sets *total = {0, 0}.
 * Kernels: the kernel of pfac_documents_group_masks, instantiated with the sum of the pair (weight, 1) in place of the
 * OR, behind a memset of the scores: a segmented add over the 64 lanes, the open run carried across chunks and tiles,
 * each document written once -- one 16-byte store where the document lies inside the wave's 64 tiles, two 64-bit atomic
 * adds for the at most two that straddle their ends.  No atomic per record. */
int pfac_documents_scores(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                          pfac_doc_score *d_scores_out, pfac_doc_score *total);
/* The same two numbers over a record array that is already cut per document: document d owns
 * d_sel[d_doc_first[d] .. d_doc_first[d + 1]), and every one of those records counts (positions are not read).
 *   d_sel, d_doc_first  both NULL = the slot-owned picks and doc_first of the slot's last
 *                  pfac_records_leftmost_longest_documents, under the rules of pfac_selection_count_states' d_sel
 *                  (PFAC_E_STATE: no such selection since the slot's last scan, a selection made with an earlier table,
 *                  or one that went to the caller's buffers).  Both non-NULL = any device arrays, 8-B aligned: the output
 *                  of pfac_records_segment, or a selection written to the caller's buffers; d_doc_first has n_docs + 1
 *                  entries and d_sel holds d_doc_first[n_docs] records (that one entry is read back first, to size
 *                  the launch).  One NULL and one not gives PFAC_E_ARG.
 * Checked on the device, in the same pass and before anything reaches a caller's buffer, else PFAC_E_ARG:
 * d_doc_first[0] == 0, d_doc_first does not decrease, every state is below num_final.  PFAC_E_STATE (no table, no state
 * weights) comes before PFAC_E_ARG (misaligned buffers, n_docs >= 2^32).  d_scores_out, *total, the slot-owned result,
 * its fetch and its lifetime are those of pfac_documents_scores: the two are ONE pass.
 * Kernels: pick-driven, one lane per record, a wave per 256 records; a record's document by a search in d_doc_first
 * between the documents of its chunk's first and last record; the segmented add and the store / atomic rule of the
 * heap kernel (a document is stored plainly where all its records lie in the wave's range). */
int pfac_selection_document_scores(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first,
                                   uint64_t n_docs, pfac_doc_score *d_scores_out, pfac_doc_score *total);
/* D2H of scores [first, first + n) of the slot-owned result of the last pfac_documents_scores /
 * pfac_selection_document_scores.  Asynchronous on the slot's stream; pfac_slot_sync completes it.  first + n > n_docs
 * gives PFAC_E_ARG; n == 0 does nothing. */
int pfac_document_scores_d2h(pfac_ctx *ctx, int slot, pfac_doc_score *host, uint64_t first, uint64_t n);
/* The documents whose score satisfies a rule.  Document d is reported iff
 *   (min_count <= count[d] <= max_count && min_score <= score[d] <= max_score && density(d)) != invert
 * (flags: 0 or PFAC_DOCS_INVERT), where density(d) is true when density_den == 0 and else
 *   score[d] * density_den >= density_num * (off[d + 1] - off[d])
 * compared exactly (two 128-bit products): "at least density_num / density_den per byte", e.g. 3 / 1000.
 *   d_scores       NULL = the slot-owned scores of the slot's last score pass (PFAC_E_STATE if there are none or they
 *                  went to the caller's buffer, PFAC_E_ARG if n_docs differs from that call's); else any device
 *                  pfac_doc_score[n_docs], 16-B aligned
 *   d_doc_offsets  read only when density_den != 0 (n_docs + 1 entries, 8-B aligned; they are not checked: a length
 *                  is off[d + 1] - off[d] as it comes); NULL = the slot's offsets, PFAC_E_STATE if it has none,
 *                  PFAC_E_ARG if n_docs differs from theirs
 *   rule           NULL gives PFAC_E_ARG
 * d_ids_out, out_cap, *n_matching, PFAC_E_OVERFLOW (exact count, nothing written), the alignment and n_docs < 2^32 are
 * exactly those of pfac_documents_matching, and the call is ONE pass with it, _context and _groups: the same slot-owned
 * id buffer, pfac_documents_matching_d2h, and pfac_documents_gather(d_ids = NULL) / _gather_format consume its ids
 * unchanged.
 * Kernels: the compaction of pfac_documents_matching, instantiated with the rule (one 16-byte load per document; with a
 * density two 8-byte loads of the offsets more). */
typedef struct {
    int64_t  min_score, max_score;      /* inclusive; INT64_MIN / INT64_MAX = not judged */
    uint64_t min_count, max_count;      /* inclusive; 0 / UINT64_MAX = not judged */
    int64_t  density_num;               /* judged only when density_den != 0 */
    uint64_t density_den;
} pfac_score_rule;
int pfac_documents_matching_scores(pfac_ctx *ctx, int slot, const pfac_doc_score *d_scores, const uint64_t *d_doc_offsets,
                                   uint64_t n_docs, const pfac_score_rule *rule, uint32_t flags, uint64_t *d_ids_out,
                                   uint64_t out_cap, uint64_t *n_matching);
/* The k best documents by score or by count, in order: "the 100 most suspicious lines", "the 20 best hits".
 *   candidates     rule == NULL: every document.  Else the documents pfac_documents_matching_scores reports for (rule,
 *                  rule_flags), density and PFAC_DOCS_INVERT included; d_doc_offsets is read only for a density, under
 *                  that call's rules.  "Matched documents only" is min_count = 1
 *   rank order     by key, ties to the smaller id.  The key is score[d], compared as signed 64-bit, largest first;
 *                  PFAC_TOP_BY_COUNT: count[d], compared as unsigned 64-bit; PFAC_TOP_LOWEST: smallest first
 *   *n_top         min(k, the number of candidates); any k up to 2^64 - 1 clamps.  k == 0 or n_docs == 0 gives 0 and
 *                  writes nothing
 *   reported       the first *n_top candidates in rank order: where k cuts through a class of equal keys, its members
 *                  with the smallest ids.  PFAC_TOP_RANKED: ids[j] is the document of rank j; else the same documents,
 *                  ids ascending (document order, as grep prints).  top_scores[j] = scores[ids[j]], the whole pair
 *   d_scores, n_docs < 2^32, the alignments and the PFAC_E_STATE / PFAC_E_ARG ladder are exactly those of
 *                  pfac_documents_matching_scores (NULL = the slot-owned scores of the slot's last score pass)
 *   d_ids_out      as in pfac_documents_matching: the call is ONE pass with it, _context, _groups and _scores -- the same
 *                  slot-owned id buffer, pfac_documents_matching_d2h, and pfac_documents_gather(d_ids = NULL) /
 *                  _gather_format consume the ids unchanged, in rank order too (the gather takes any order)
 *   d_top_scores_out  NULL = a slot-owned buffer of its own (pfac_documents_top_scores_d2h; the lifetime rule of
 *                  pfac_segment_d2h: the next pfac_documents_top_scores discards it, a matching call does not); else a
 *                  device pointer, 16-B aligned, out_cap entries like d_ids_out
 * PFAC_E_OVERFLOW with *n_top exact when out_cap < *n_top and either output is the caller's; PFAC_E_ARG also for flags
 * outside the three and rule_flags outside PFAC_DOCS_INVERT.  Every error leaves every caller's buffer untouched; a
 * failed call discards the slot-owned ids and pairs.  No entry at or past *n_top is written in either output: buffers
 * of exactly *n_top x 8 and *n_top x 16 bytes are enough.  Returns once *n_top is known (one 8-byte copy back); the
 * writes complete on the slot's stream.  The same call on the same scores gives the same bytes.
 * A rank by DENSITY (score per byte) is out of scope: a ratio has no radix key.  A density only filters.
 * Kernels: (1) an MSB-first radix select of the key of rank *n_top over an order-preserving 64-bit word (sign bit
 * flipped for scores, all bits inverted for "largest first"): eight passes of 8 bits, each a grid-stride read of the
 * pairs into LDS histograms (lanes that agree on the digit are found by ballots and add once) flushed with 64-bit
 * atomics; the digit that holds the rank is chosen on the device, by every wave of the next pass from the small
 * histogram; the first pass counts the candidates.  (2) The compaction of pfac_documents_matching with two counts per
 * block and group -- keys in front of the threshold key T, keys equal to T -- which takes every candidate in front of T
 * and the first `need` of those equal to it, ascending, and writes the pairs in the same pass.  (3) PFAC_TOP_RANKED: a
 * stable LSD radix sort of the *n_top (key word, id) entries, ranks inside a wave from ballots; stability is the tie
 * rule, since step 2 delivers ascending ids.  Up to PFAC_TOP_SORT_BLOCK entries it is one workgroup working in LDS,
 * above that blocks of PFAC_TOP_SORT_BLOCK with a histogram, a prefix and a scatter per pass between two scratch
 * buffers.  The last pass writes the ids and gathers the pairs. */
#define PFAC_TOP_BY_COUNT  1u   /* key = count[d] (uint64); default key = score[d] (int64, signed order) */
#define PFAC_TOP_LOWEST    2u   /* the k smallest keys instead of the k largest */
#define PFAC_TOP_RANKED    4u   /* ids in rank order; default: the same ids, ascending (document order, as grep prints) */
#define PFAC_TOP_SORT_BLOCK 1024u   /* entries per workgroup of the ranked sort, and the most that one workgroup sorts alone */
int pfac_documents_top_scores(pfac_ctx *ctx, int slot, const pfac_doc_score *d_scores, const uint64_t *d_doc_offsets,
                              uint64_t n_docs, const pfac_score_rule *rule, uint32_t rule_flags, uint64_t k, uint32_t flags,
                              uint64_t *d_ids_out, uint64_t out_cap, pfac_doc_score *d_top_scores_out, uint64_t *n_top);
/* D2H of pairs [first, first + n) of the slot-owned result of the last pfac_documents_top_scores.  Asynchronous on the
 * slot's stream; pfac_slot_sync completes it.  first + n > *n_top gives PFAC_E_ARG; n == 0 does nothing. */
int pfac_documents_top_scores_d2h(pfac_ctx *ctx, int slot, pfac_doc_score *host, uint64_t first, uint64_t n);
/* Term counts per document: WHICH final states each document holds and how often -- the document-term matrix (the
 * bag-of-words vector of every line under a dictionary) as the three arrays of a CSR matrix, which
 * torch.sparse_csr_tensor takes as they are.  The input is a record array that is already cut per document: document d
 * owns d_sel[d_doc_first[d] .. d_doc_first[d + 1]); positions are not read.
 *   d_sel, d_doc_first  both non-NULL = any device arrays, 8-B aligned: the caller's output of pfac_records_segment or of
 *                  the per-document selection; d_doc_first has n_docs + 1 entries and d_sel holds d_doc_first[n_docs]
 *                  records (that one entry is read back first, to size the launch).  Both NULL, flags 0 = the
 *                  slot-owned records and doc_first of the slot's last pfac_records_segment (PFAC_E_STATE: none, it
 *                  went to the caller's buffers, or it was cut with an earlier table).  Both NULL,
 *                  PFAC_TERMS_SELECTION = the slot-owned picks and doc_first of the slot's last
 *                  pfac_records_leftmost_longest_documents, under the rules of pfac_selection_count_states' d_sel
 *                  (PFAC_E_STATE: no such selection since the slot's last scan, one made with an earlier table, or one
 *                  that went to the caller's buffers).  Both NULL with an n_docs that is not that call's gives
 *                  PFAC_E_ARG; so does one NULL and one not.
 *   n_docs < 2^32, and the record count N = d_doc_first[n_docs] < 2^32 (every count fits 32 bits), else PFAC_E_ARG
 *   result         let U be the distinct (d, state) pairs over all records, in (d, state) order: *n_terms = |U|,
 *                  states[j] and counts[j] are the state and the multiplicity of the j-th pair, row_ptr[d] = the pairs
 *                  whose document is < d (row_ptr[0] = 0, row_ptr[n_docs] = *n_terms).  Within a document the states
 *                  strictly ascend; an empty or unmatched document has row_ptr[d + 1] == row_ptr[d].  A state is a
 *                  final state, as in pfac_records_count_states: the host turns states into pattern ids
 *   d_row_ptr_out  NULL = a slot-owned buffer grown to fit; else a device pointer, 8-B aligned, n_docs + 1 entries
 *   d_states_out, d_counts_out  each NULL = a slot-owned buffer grown to fit; else device pointers, 4-B aligned,
 *                  out_cap entries each
 * Checked on the device, before anything reaches a caller's buffer, else PFAC_E_ARG: d_doc_first[0] == 0, d_doc_first
 * does not decrease, every state is below num_final of the uploaded table.  PFAC_E_STATE (no table; a slot-owned input
 * that is missing, stale or from an earlier table) comes before PFAC_E_ARG (misaligned buffers, n_docs >= 2^32,
 * N >= 2^32, flags outside 0..1).  PFAC_E_OVERFLOW with *n_terms exact when out_cap < *n_terms and either of the two
 * entry arrays is the caller's.  Every error leaves every caller's buffer of the call untouched, d_row_ptr_out
 * included.  Nothing at or past *n_terms is written in the entry arrays and nothing at or past n_docs + 1 in row_ptr:
 * buffers of exactly (n_docs + 1) x 8, *n_terms x 4 and *n_terms x 4 bytes are enough.  n_docs == 0 writes the single
 * row_ptr[0] = 0; N == 0 writes n_docs + 1 zeros and no entries.
 * A pass of its own, with the lifetime rule of pfac_segment_d2h: it discards no other pass's result and is discarded by
 * none; a failed call discards its own slot-owned result.  Returns once *n_terms is known (one small copy back: the
 * total and the error word); the writes complete on the slot's stream.  The same call on the same input gives the same
 * bytes.  It reads neither the input bytes nor the record heap.
 * Kernels: (1) one lane per record, a wave per 256 records: the record's document by a search in d_doc_first bounded by
 * its chunk's first and last record, the three checks, and the 8-byte key doc << sbits | state with sbits =
 * bit_width(num_final - 1) -- packed, so that (2) a stable LSD radix sort of the keys runs ceil((sbits +
 * bit_width(n_docs - 1)) / 8) passes of 8 bits and no more; ranks inside a wave from ballots; a workgroup takes as
 * many consecutive chunks of PFAC_TERMS_SORT_BLOCK keys per histogram row as keep a pass within PFAC_TERMS_SORT_ROWS
 * workgroups, and the prefix of a pass is one workgroup per digit over that digit's row; up to PFAC_TERMS_SORT_BLOCK
 * keys are sorted by one workgroup in LDS.  The key is document-major: document d's records still lie in
 * [doc_first[d], doc_first[d + 1]).
 * (3) Entry i is a head iff i == 0 or key[i] != key[i - 1]: heads per block of 64 and per group of 4096, the group
 * prefix, and every block's 64-bit head ballot kept.  (4) Behind the host's overflow check every head of rank j stores
 * states[j] and its index; counts[j] is the difference of two neighbouring head indices, and row_ptr[d] is three loads
 * and a popcount at entry doc_first[d] -- no loop runs as long as a run of equal records or of empty documents. */
#define PFAC_TERMS_SELECTION 1u   /* d_sel == d_doc_first == NULL means the slot's per-document selection, not its segment result */
#define PFAC_TERMS_SORT_BLOCK 1024u   /* keys per chunk of the sort, and the most that one workgroup sorts alone */
#define PFAC_TERMS_SORT_ROWS  4096u   /* the most workgroups (histogram rows per digit) of one sort pass */
int pfac_documents_term_counts(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first,
                               uint64_t n_docs, uint32_t flags,
                               uint64_t *d_row_ptr_out, uint32_t *d_states_out, uint32_t *d_counts_out, uint64_t out_cap,
                               uint64_t *n_terms);
/* D2H of the slot-owned result of the last pfac_documents_term_counts: n_docs + 1 row_ptr entries, *n_terms states and
 * *n_terms counts.  Any of the three may be NULL (it must be where that output was the caller's: PFAC_E_STATE else).
 * Asynchronous on the slot's stream; pfac_slot_sync completes it. */
int pfac_documents_term_counts_d2h(pfac_ctx *ctx, int slot, uint64_t *host_row_ptr, uint32_t *host_states,
                                   uint32_t *host_counts);

/* Rule sets: WHICH of many rules fired in each document -- the several content: strings of a Snort rule that must all
 * occur, YARA's "all of them", "2 of ($a, $b, $c)" and "$a and not $b", the words of a label rule -- for thousands of
 * rules over tens of thousands of patterns at once, where the group masks allow 64 classes and one predicate per call.
 * It is the join of the document-term matrix (pfac_documents_term_counts) with a rule table.
 *
 * The table (pfac_table_set_rules).  Rule r has a set P_r of positive final states, a set N_r of negated ones, disjoint
 * from P_r, and need_r with 1 <= need_r <= |P_r|.  With S_d the states of row d of the matrix,
 *   rule r fires in document d iff |P_r & S_d| >= need_r and N_r & S_d is empty.
 * need = |P| is AND, need = 1 is OR, anything between "k of them".  A rule without a positive term cannot be stated, so
 * only documents with a record can fire.
 *   rule_ptr, terms, need  HOST arrays, rule-major, copied at the call: terms[rule_ptr[r] .. rule_ptr[r + 1]) are rule r's
 *                  final states, bit 31 (PFAC_RULE_NOT) marks a negated one; need[r].  n_rules < 2^31 and fewer than
 *                  2^32 terms in all.  n_rules == 0 is legal (the pointers may be NULL) and clears the rules only
 * PFAC_E_STATE before a table upload.  PFAC_E_ARG, with the earlier rules kept: rule_ptr[0] != 0 or a decrease, a state at
 * or past num_final, a state twice in one rule (under either sign), need == 0 or need above the rule's positive terms.
 * The host inverts the table to state-major (state_ptr uint32[num_final + 1]; entries rule << 1 | negated, the rules
 * ascending inside a state; need[]) and uploads it under the lifetime rules of pfac_table_set_state_groups: the arrays
 * live with the table, an upload clears them, a second call replaces them, and freeing the old buffers waits for the
 * device, so a pass that still reads them has finished.
 *
 * The pass (pfac_documents_rules).
 *   d_row_ptr, d_states  both non-NULL = any device arrays, 8-B and 4-B aligned: the first two arrays of a document-term
 *                  matrix as pfac_documents_term_counts writes them (the counts are not read); d_row_ptr has n_docs + 1
 *                  entries and d_row_ptr[n_docs] is read back first, to size the launch.  Both NULL = the slot-owned
 *                  row_ptr and states of the slot's last pfac_documents_term_counts (PFAC_E_STATE: none, either went to
 *                  the caller's buffer, or it was made with an earlier table; an n_docs that is not that call's gives
 *                  PFAC_E_ARG).  One NULL and one not gives PFAC_E_ARG
 *   flags          0
 *   result         a CSR of fired rules: row_ptr uint64[n_docs + 1] and rules uint32[*n_fired], a document's rule ids
 *                  strictly ascending
 *   d_row_ptr_out  NULL = a slot-owned buffer grown to fit; else a device pointer, 8-B aligned, n_docs + 1 entries
 *   d_rules_out    NULL = a slot-owned buffer grown to fit; else a device pointer, 4-B aligned, out_cap entries
 * Checked on the device, before anything reaches a caller's buffer, else PFAC_E_ARG: d_row_ptr[0] == 0, d_row_ptr does
 * not decrease, every state is below num_final, the states strictly ascend inside a row.  Judged in this order --
 * PFAC_E_STATE: no table, no rules for it, a slot-owned input that is missing or from an earlier table; PFAC_E_ARG: one
 * input NULL and the other not, flags other than 0, misaligned buffers, n_docs >= 2^32, 2^32 or more pairs, the device's
 * checks, and an expansion E >= 2^32, where E = the sum over all pairs of the rules that name the pair's state.
 * PFAC_E_OVERFLOW with *n_fired exact when out_cap < *n_fired and d_rules_out is the caller's.  Every error leaves every
 * caller's buffer untouched; exactly (n_docs + 1) x 8 and *n_fired x 4 bytes are written.  n_docs == 0 writes the single
 * row_ptr[0] = 0.
 * A pass of its own, with the lifetime rule of pfac_segment_d2h: it discards no other pass's result and is discarded by
 * none; a failed call discards its own slot-owned result.  Returns once *n_fired is known (two small copies back: E with
 * the error word, then the total); the writes complete on the slot's stream.  The same call on the same input gives the
 * same bytes.  It reads neither the input bytes, nor the record heap, nor the cut records.
 * Kernels: (1) one lane per pair, a wave per 4096 pairs: the pair's document by a search in d_row_ptr bounded by its
 * block's first and last pair, c = state_ptr[s + 1] - state_ptr[s], the four checks into one word; kept per pair its
 * document and the entries in front of it in its group, per group the sum, then the group prefix: E is the total, and
 * E == 0 writes zeros without a further launch.  (2) Output-driven, one lane per key e < E: its group and its pair by two
 * searches in the prefixes, then its entry: key = doc << (rbits + 1) | rule << 1 | negated, rbits = bit_width(n_rules -
 * 1) -- no loop is as long as a state's rule count.  (3) The stable LSD sort of pfac_documents_term_counts (the same
 * kernels, PFAC_TERMS_SORT_ROWS and its knob) over ceil((bit_width(n_docs - 1) + rbits + 1) / 8) digits.  (4) A (document,
 * rule) run is now contiguous, its positive entries in front of its negated ones, every entry another term: entry t is
 * a tail iff t == E - 1 or key[t + 1] >> 1 != key[t] >> 1, and the run fires iff key[t] & 1 == 0, t >= need - 1 and
 * key[t - (need - 1)] >> 1 == key[t] >> 1 -- one more load per tail, no head ranks, no run lengths; a ballot per 64
 * entries is kept, the sums per 4096 go through the group prefix.  (5) Behind the host's overflow check the fired tail of
 * rank j stores rules[j]; row_ptr[d] is a lower bound of d << (rbits + 1) in the sorted keys, two loads and a popcount. */
#define PFAC_RULE_NOT 0x80000000u   /* bit 31 of a term: the rule must NOT find this state in the document */
int pfac_table_set_rules(pfac_ctx *ctx, const uint64_t *rule_ptr, const uint32_t *terms, const uint32_t *need,
                         uint64_t n_rules);
int pfac_documents_rules(pfac_ctx *ctx, int slot, const uint64_t *d_row_ptr, const uint32_t *d_states, uint64_t n_docs,
                         uint32_t flags, uint64_t *d_row_ptr_out, uint32_t *d_rules_out, uint64_t out_cap,
                         uint64_t *n_fired);
/* D2H of the slot-owned result of the last pfac_documents_rules: n_docs + 1 row_ptr entries and *n_fired rule ids.
 * Either may be NULL (it must be where that output was the caller's: PFAC_E_STATE else).  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it. */
int pfac_documents_rules_d2h(pfac_ctx *ctx, int slot, uint64_t *host_row_ptr, uint32_t *host_rules);

/* Proximity rules: WHERE the pattern groups of a document occur relative to each other -- a card number within 60 bytes
 * of "expires", the within: of two contents of one rule, NEAR/n, "BEGIN before END on the same line".  The group masks
 * say that both halves occur in a document; this pass says that they occur together, and in which order.  The classes
 * are the state groups (pfac_table_set_state_groups); the input is a record array that is already cut per document,
 * exactly as pfac_documents_term_counts takes it -- but here the positions are read.
 *   d_sel, d_doc_first  both non-NULL = the caller's device arrays, 8-B aligned (d_doc_first[n_docs] is read back first,
 *                  to size the launch); both NULL, flags 0 = the slot-owned result of the slot's last
 *                  pfac_records_segment; both NULL, PFAC_NEAR_SELECTION = the slot-owned per-document selection --
 *                  under the staleness rules of pfac_documents_term_counts (PFAC_E_STATE), and both NULL with an n_docs
 *                  that is not that call's, or one NULL and one not, gives PFAC_E_ARG.  n_docs < 2^32 and
 *                  N = d_doc_first[n_docs] < 2^32.  Within a document the positions must not decrease: both producers
 *                  guarantee it, and it holds for document-relative positions (the segment pass) and stream-relative
 *                  ones (the selection) alike, because only differences inside one document are used
 *   rules          HOST array of n_rules <= PFAC_NEAR_MAX_RULES rules, copied at the call (the caller may free it when
 *                  the call returns).  With A_r(i) = groups[state_i] & a_groups != 0 and B_r likewise,
 *   rule r fires in document d iff there are two DISTINCT records i < j in [doc_first[d], doc_first[d + 1]) with
 *                  pos[j] - pos[i] <= max_dist and
 *                    ordered (PFAC_NEAR_ORDERED):  A_r(i) && B_r(j)
 *                    unordered:                    (A_r(i) && B_r(j)) || (B_r(i) && A_r(j))
 *   result         mask[d] has bit r set iff rule r fired in d; a document without records gets 0; *any_mask is the OR
 *                  of all masks.  n_rules == 0 gives all-zero masks
 *   d_masks_out    NULL = a slot-owned buffer grown to fit (pfac_near_masks_d2h, pfac_slot_near_masks); else a device
 *                  pointer, 8-B aligned: exactly n_docs x 8 bytes are written
 * Two decisions.  "Precedes" (i < j) is the order of the record array, which is (position, pattern length): at equal
 * starts the shorter pattern is the earlier record, so an ordered rule whose A and B start at one byte fires iff the A
 * is the shorter; unordered rules do not depend on it, and over the selection no two records share a start.  And a
 * record never pairs with itself: A and B may overlap, and a rule with a_groups == b_groups means "two occurrences
 * within max_dist".  max_dist is the start-to-start distance in bytes, inclusive; 0 is legal (two records at one
 * start); PFAC_NEAR_ANY_DIST makes an ordered rule "an A somewhere before a B in this document".  A rule whose a_groups
 * or b_groups is 0 never fires.  Not in the rule, on purpose: a minimum distance, and distances measured from the END
 * of A -- with a maximum only the nearest earlier partner is always the best one, which is what keeps the pass at
 * O(N x n_rules).
 * Judged in this order -- PFAC_E_STATE: no table, no state groups for the current table, a slot-owned input that is
 * missing, stale or from an earlier table; PFAC_E_ARG: misaligned buffers, one input NULL and the other not, call flags
 * outside 0..1, an n_docs that is not the slot-owned input's, n_docs or N >= 2^32, n_rules > 64, rules == NULL with
 * n_rules > 0, a rule with flags outside 0..1 or reserved != 0; and, checked on the device: d_doc_first[0] != 0, a
 * d_doc_first that decreases, a state at or above num_final, a position that decreases inside a document.  Every error
 * leaves a caller's d_masks_out untouched (the masks are made in the slot's buffer and copied behind the host's check,
 * as pfac_documents_group_masks does).  n_docs == 0 writes nothing and sets *any_mask = 0.
 * A pass of its own, with the lifetime rule of pfac_segment_d2h: it discards no other pass's result and is discarded by
 * none; a failed call discards its own slot-owned result.  Returns once *any_mask and the error word are known (one
 * 16-byte copy back); the masks are then complete on the slot's stream.  The same call on the same input gives the same
 * bytes.
 * Kernels, over blocks of 4096 records: (1) one wave per block writes, per rule and side, the index and position of
 * the block's last A / last B -- walking its chunks of 64 from the end, and only for the rules still without one;
 * (2) one workgroup per (rule, side) turns those into every block's carry-in, an exclusive "last non-empty"; (3) the
 * pass, one wave per block and one read of the records: per chunk of 64 a lane loads its record, gathers its groups and
 * finds its document by a search in d_doc_first bounded by the chunk's ends; per rule two ballots, the lane's last
 * earlier partner from the ballot's bits below the lane (its position by one lane permute) or, with none in the chunk,
 * from the rule's carry, which lane r keeps for rule r; the fired bits of a lane are one word, ORed per document by the
 * segmented scan of the group-mask kernel: a plain 8-byte store for a document inside the block, an atomic OR for the
 * at most two that straddle its ends, behind a memset.  No atomic per record, no scratch proportional to N x n_rules
 * (the table holds N / 4096 x n_rules x 2 entries), no walk over "the records inside the window". */
#define PFAC_NEAR_MAX_RULES 64u
#define PFAC_NEAR_ORDERED   1u            /* rule flag: the A record precedes the B record in record order */
#define PFAC_NEAR_ANY_DIST  0xFFFFFFFFu   /* max_dist: anywhere in the same document */
typedef struct pfac_near_rule {           /* 32 bytes */
    uint64_t a_groups;         /* a record is an A of this rule iff groups[state] & a_groups */
    uint64_t b_groups;         /* ... a B iff groups[state] & b_groups; A and B may overlap */
    uint32_t max_dist;         /* start-to-start distance in bytes, inclusive */
    uint32_t flags;            /* 0 or PFAC_NEAR_ORDERED */
    uint64_t reserved;         /* must be 0 */
} pfac_near_rule;
#define PFAC_NEAR_SELECTION 1u   /* call flag: d_sel == d_doc_first == NULL means the slot's per-document selection, as PFAC_TERMS_SELECTION */
int pfac_documents_near(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first, uint64_t n_docs,
                        uint32_t flags, const pfac_near_rule *rules, uint32_t n_rules, uint64_t *d_masks_out,
                        uint64_t *any_mask);
/* D2H of masks [first, first + n) of the slot-owned result of the last pfac_documents_near.  Asynchronous on the slot's
 * stream; pfac_slot_sync completes it.  first + n > n_docs gives PFAC_E_ARG; n == 0 does nothing. */
int pfac_near_masks_d2h(pfac_ctx *ctx, int slot, uint64_t *host_masks, uint64_t first, uint64_t n);
/* Device pointer of those slot-owned masks (uint64[n_docs]; what pfac_documents_matching_groups takes as d_masks), NULL
 * if there are none: no finished call, or its masks went to the caller's buffer.  Valid until the slot's next
 * pfac_documents_near. */
void *pfac_slot_near_masks(pfac_ctx *ctx, int slot);

/* Whole-word filter: drops, IN PLACE, the records of the slot's last finished scan that split a word, so that every
 * consumer of the scan (the fetches, the text emitter, the checksum, the segment pass, both selections and both
 * replaces) sees whole-word matches only -- a selection then chooses among whole-word candidates, which no filter
 * behind it could repair.  The scan kernel is not involved.
 *   W(b)   = bit b of word_set: a 256-bit set, byte b at bit (b & 63) of word_set[b >> 6].  NULL = [0-9A-Za-z_]
 *            (a UTF-8 user also sets 0x80..0xFF).
 *   in[i]  = the scanned buffer for 0 <= i < n_avail; in[-1] = prev_byte and in[n_avail] = next_byte, each -1 (no byte:
 *            the text starts / ends there) or 0..255 -- what makes chained ranges exact.
 *   cut(i) = in[i-1] and in[i] both exist and are word bytes; with documents, and i is none of the document offsets.
 *   A record (pos, state), L = the final length of state, is KEPT iff
 *            !((edges & PFAC_WORD_LEFT) && cut(pos)) && !((edges & PFAC_WORD_RIGHT) && cut(pos + L)).
 * So a pattern that begins (ends) with a non-word byte is unconstrained on that side, and for patterns of word bytes
 * only LEFT | RIGHT is (?<!\w)pat(?!\w).  pos + L <= n_avail holds for every record: input reads stay in [0, n_avail).
 * Effect: every tile's kept words are compacted to the front of the tile's own run of the heap, order preserved;
 * tile_index[t] keeps its FIRST and gets the new COUNT; *n_kept becomes the scan's match count for everything that
 * follows -- a repeated pfac_scan_finish, the first + n bounds of pfac_records_expand / pfac_records_d2h, the n of the
 * checksum, the text emitter, every pass.  used, record_bytes and n_tiles of pfac_scan_format do not change, and no byte
 * outside the words the scan itself wrote is written.  Filtering again with the same arguments changes nothing; other
 * arguments compose (the intersection).  A selection made before the filter is stale: pfac_replace_* return
 * PFAC_E_STATE for it, as after a new scan.  Slot-owned results of earlier passes stay fetchable (the lifetime rule
 * of pfac_segment_d2h), and so does the text of an earlier pfac_emit_text_device, as it was emitted.  The filter belongs
 * to the scan it ran on: the slot's next scan reports its own full count, and the other slots are not touched.
 *   d_input        NULL = the slot's input buffer; else the buffer the scan read (16-B aligned)
 *   d_records      NULL = the slot's heap; else the heap the scan wrote (any other pointer: PFAC_E_ARG)
 *   n_docs         0 = no documents.  Else the rules of pfac_records_segment hold for d_doc_offsets (NULL = the slot's,
 *                  pfac_slot_doc_offsets with the same n_docs, else PFAC_E_STATE); they are checked on the device in
 *                  front of the filter, whose kernel reads the check's flag and leaves at once: a violation returns
 *                  PFAC_E_ARG with heap, index and count untouched, at no extra host round trip.  A record that runs
 *                  across a document end is judged like any other (the document passes drop it later, as ever).
 * Returns once *n_kept is known.  PFAC_E_ARG: edges outside 1..3, prev_byte / next_byte outside -1..255, a d_records
 * that is not this scan's heap, a misaligned d_input.  PFAC_E_STATE: no finished scan (also after a pfac_slot_reserve
 * that dropped it), a scan made with an earlier table, no final lengths for the current table.  PFAC_E_OVERFLOW: the
 * scan overflowed its heap.  A call that breaks several rules: the scan's state is judged before the arguments
 * (PFAC_E_STATE, then PFAC_E_OVERFLOW, then the rest); among the arguments no order is promised, except that offsets
 * whose n_docs is not the slot's are not looked at (PFAC_E_STATE).  Every error leaves heap, index, count, and what a
 * selection made before may still be used for, as they were.
 * Kernel: one wave per tile at a time, 64 tiles per wave; per chunk of 64 records the record, its length, up to four
 * byte gathers (pos - 1, pos, pos + L - 1, pos + L), a ballot, and the kept words stored at FIRST + kept + rank -- at or
 * below the chunk's own slots, after all of the chunk's loads, so no later chunk is overwritten before it is read. */
#define PFAC_WORD_LEFT  1u   /* the match must not begin inside a word */
#define PFAC_WORD_RIGHT 2u   /* the match must not end inside a word   */
int pfac_records_filter_words(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, const uint64_t word_set[4],
                              uint32_t edges, int prev_byte, int next_byte, const uint64_t *d_doc_offsets, uint64_t n_docs,
                              uint64_t *n_kept);

/* Spans: WHERE in its document (line) a pattern may match -- ^pat, pat$, grep -x, the offset / depth qualifiers of a
 * content rule.  One span per final state of the uploaded table; PFAC_SPAN_ANY is "not bounded".  n_states must be
 * num_final, and every `reserved` 0, else PFAC_E_ARG and the earlier spans stay; PFAC_E_STATE before a table upload.
 * The spans live on the device with the table, like the state groups: the next pfac_table_upload / _upload_device clears
 * them, a second call replaces them.  The call waits for no scan; a filter already queued keeps the spans it was launched
 * with (the old buffer is freed behind it). */
#define PFAC_SPAN_ANY 0xFFFFFFFFu
typedef struct pfac_state_span {   /* 16 bytes: one dwordx4 gather per record */
    uint32_t min_start;            /* rel >= min_start                                  (Snort offset) */
    uint32_t max_start;            /* rel <= max_start   (0: ^;  offset + depth - L)                   */
    uint32_t max_tail;             /* tail <= max_tail   (0: $);  PFAC_SPAN_ANY: not judged            */
    uint32_t reserved;             /* must be 0, else PFAC_E_ARG                                       */
} pfac_state_span;
int pfac_table_set_state_spans(pfac_ctx *ctx, const pfac_state_span *spans, uint64_t n_states);
/* Span filter: the positional sibling of pfac_records_filter_words.  Drops, IN PLACE, the records of the slot's last
 * finished scan whose state's span does not admit them, so that every consumer of the scan sees the admissible matches
 * only, and a selection chooses among them.  The scan kernel is not involved.
 * The rule.  A record (pos, s), L = the final length of s.  With documents (n_docs > 0; d_doc_offsets under the rules of
 * pfac_records_segment), d is the last document with off[d] <= pos; n_docs == 0 means ONE document [0, n_avail).  Then
 *   rel  = pos - off[d],  E = off[d + 1]
 *   C    = E - 1 if delimiter >= 0 and E > off[d] and in[E - 1] == delimiter, else C = E
 *          (a line keeps its delimiter, so `$` sits in front of it)
 *   tail = C - (pos + L)  if pos + L <= C
 *        = 0              if C < pos + L <= E   (the match covers the delimiter: `foo\n` from an escaped file)
 *        = infinite       if pos + L > E        (a record that runs across its document's end fails every max_tail other
 *                                                than PFAC_SPAN_ANY; its start rule is judged as usual)
 *   the record is KEPT iff  min_start <= rel <= max_start && (max_tail == PFAC_SPAN_ANY || tail <= max_tail).
 * flags & PFAC_SPANS_LINE judges every state as {0, 0, 0} -- grep -x -- and needs no spans set.
 * Input reads: in[E - 1] alone, only for a record whose max_tail is judged, only when delimiter >= 0.  E <= n_owned <=
 * n_avail, so no byte at or past n_avail is read.  With delimiter == -1 d_input is ignored and the input is never read.
 * Under a folded scan the bytes are read as they are (the scan never writes its input), as in the whole-word filter.
 * Effect, as pfac_records_filter_words: every tile's kept words are compacted to the front of the tile's own run of the
 * heap, order preserved; tile_index[t] keeps its FIRST and gets the new COUNT; *n_kept becomes the scan's match count
 * for everything that follows.  used, record_bytes and n_tiles of pfac_scan_format do not change, and no byte outside
 * the words the scan itself wrote is written.  A selection made before the call is stale (pfac_replace_* return
 * PFAC_E_STATE).  Filtering again with the same arguments changes nothing.  The filter composes with the whole-word
 * filter in either order: the result is the intersection.
 *   d_input        NULL = the slot's input buffer; else the buffer the scan read (16-B aligned); ignored without delimiter
 *   d_records      NULL = the slot's heap; else the heap the scan wrote (any other pointer: PFAC_E_ARG)
 *   delimiter      -1 = none (C = E), else the byte 0..255 that ends a line
 *   n_docs         0 = one document [0, n_avail).  Else d_doc_offsets (NULL = the slot's, with the same n_docs) are
 *                  checked on the device in front of the filter, whose kernel reads the check's flag and leaves at once.
 * Returns once *n_kept is known.  Judged in this order -- PFAC_E_STATE: no finished scan, a scan made with an earlier
 * table, no final lengths, no spans for the current table (unless PFAC_SPANS_LINE is set), an n_docs that is not that
 * of the slot's offsets; PFAC_E_OVERFLOW: the scan overflowed its heap; PFAC_E_ARG: delimiter outside -1..255, flags
 * outside 0..1, a misaligned d_input, a d_records that is not this scan's heap, offsets that break the rules.  Every
 * error leaves heap, index and count as they were.
 * Kernel: the walk of the whole-word filter (one wave per tile at a time, 64 tiles per wave); per chunk of 64 records the
 * record, its length, its span (one 16-byte gather; registers and shuffles for tables of at most 64 final states;
 * nothing under PFAC_SPANS_LINE), its document, a ballot, and the kept words stored at FIRST + kept + rank. */
#define PFAC_SPANS_LINE 1u         /* every state judged as {0, 0, 0}: grep -x; needs no spans set */
int pfac_records_filter_spans(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, int delimiter,
                              uint32_t flags, const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t *n_kept);

/* Leftmost-longest, non-overlapping selection over the slot's last finished scan.  From a cursor c = entry
 * (0 <= entry <= max_pat_len of the uploaded table): take the smallest position p >= c that has a record, select its
 * record of the greatest pattern length (the last one at p), set c = p + len, repeat while records remain at or after c.
 *   d_records   the scan's record heap, NULL = the slot's
 *   d_out       NULL = a slot-owned buffer grown to fit (fetched with pfac_leftmost_longest_d2h); else a device pointer,
 *               8-B aligned, holding out_cap records.  The selection is written as {pos, state} in ascending pos,
 *               positions relative to the scan's start (as pfac_records_d2h).
 *   *exit_offset = max(c_final, n_owned) - n_owned, c_final the cursor after the last pick (entry if none): in
 *               [0, max_pat_len].  Passed as the next scan's entry, scans chained over consecutive owned ranges (with
 *               the usual max_pat_len - 1 halo) select exactly what one scan of the whole range selects.
 * Needs the final-state lengths of the current table (pfac_table_set_final_lengths).
 * Returns once *n_selected and *exit_offset are known; the writes are asynchronous on the slot's stream.
 * PFAC_E_OVERFLOW (with *n_selected exact, nothing written) when out_cap is too small for a caller's d_out;
 * PFAC_E_ARG for entry > max_pat_len or misaligned buffers; PFAC_E_STATE without a finished scan, for a scan made with
 * an earlier table, without lengths for the current table, or when the scan overflowed its heap.
 * Kernels: every tile of 4 KiB is a function from its entry offset to its exit offset (the cursor that reaches a tile
 * lies within max_pat_len of its start); one pass builds them per group of 64 tiles, two small ones compose the groups
 * and evaluate them from entry, a second pass marks every tile's picks, then the group prefix and the write.  They read
 * the record heap, the tile index and the lengths, never the input.  The slot-owned output is separate from
 * pfac_records_segment's. */
int pfac_records_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_records, uint32_t entry, pfac_record *d_out,
                                  uint64_t out_cap, uint64_t *n_selected, uint32_t *exit_offset);
/* D2H of the slot-owned result of the last pfac_records_leftmost_longest (*n_selected records).  Asynchronous on the
 * slot's stream; pfac_slot_sync completes it. */
int pfac_leftmost_longest_d2h(pfac_ctx *ctx, int slot, pfac_record *host);

/* Leftmost-longest selection per document: the slot's last finished scan cut into documents [off[d], off[d+1]) (the
 * rules of pfac_records_segment), and every document given its own leftmost-longest selection from cursor 0 over the
 * records that end inside it (pos + len <= off[d+1]): what pfac_records_leftmost_longest of each document scanned on
 * its own selects.  The kernels run the selection above over the whole scan from entry 0 with one change: at a
 * position p of document d the candidate is the longest record at p that ends at or before off[d+1].  No candidate
 * crosses a document end, so the cursor never passes a document start and the selection restarts at every document.
 *   d_records      the scan's record heap, NULL = the slot's
 *   d_doc_offsets  device uint64[n_docs + 1], NULL = the slot's (pfac_slot_doc_offsets, same n_docs); the rules of
 *                  pfac_records_segment (off[0] == 0, non-decreasing, off[n_docs] == n_owned, n_docs < 2^32)
 *   d_out          the selection as {pos, state} in ascending pos, pos RELATIVE TO THE SCAN (not the document); NULL =
 *                  the slot-owned selection buffer of pfac_records_leftmost_longest; else 8-B aligned, out_cap records
 *   d_doc_first    d_doc_first[d] = index of document d's first pick, d_doc_first[n_docs] = *n_selected; NULL = a
 *                  slot-owned buffer (fetched with pfac_leftmost_longest_documents_d2h); else 8-B aligned, n_docs + 1
 * The call is the slot's last selection, with entry 0 and exit 0: pfac_replace_leftmost_longest consumes it unchanged
 * (and returns the documents' outputs concatenated), pfac_replace_documents adds the per-document output offsets.
 * Returns once *n_selected is known; the writes are asynchronous on the slot's stream.  PFAC_E_OVERFLOW (with
 * *n_selected exact, nothing written) when out_cap is too small for a caller's d_out; PFAC_E_ARG for offsets that break
 * the rules (checked on the device in the first pass, nothing written) or misaligned buffers; PFAC_E_STATE as
 * pfac_records_leftmost_longest, or without offsets for the slot.
 * Kernels: those of pfac_records_leftmost_longest, the two tile passes in a document form (each tile finds a record's
 * document in a window of the offsets: lane shuffles when fewer than 63 documents start in it, else a binary search in
 * memory), and a document write that also fills d_doc_first from the tiles' pick bitmaps. */
int pfac_records_leftmost_longest_documents(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets,
                                            uint64_t n_docs, pfac_record *d_out, uint64_t out_cap, uint64_t *d_doc_first,
                                            uint64_t *n_selected);
/* D2H of the slot-owned result of the last pfac_records_leftmost_longest_documents (host_records: *n_selected records,
 * may be NULL when d_out was the caller's; host_doc_first: n_docs + 1 entries, may be NULL when d_doc_first was the
 * caller's).  Asynchronous on the slot's stream; pfac_slot_sync completes it. */
int pfac_leftmost_longest_documents_d2h(pfac_ctx *ctx, int slot, pfac_record *host_records, uint64_t *host_doc_first);

/* Find-and-replace over the leftmost-longest selection.  Every final state s gets a replacement: bytes[offsets[s] ..
 * offsets[s+1]) (offsets holds n_states + 1 ascending entries, the last <= n_bytes < 2^32; n_states must equal num_final
 * of the uploaded table, else PFAC_E_ARG).  One replacement is at most PFAC_MAX_REPLACEMENT bytes (else PFAC_E_ARG).
 * The replacement of a pattern id goes to its state through idmap: for duplicate lines the state of the line that wins,
 * for character-class tables the state's first (lowest) id; unreachable states may be empty.  Kept on the device until
 * the next table upload clears them, like the final lengths. */
#define PFAC_MAX_REPLACEMENT 65536u
int pfac_table_set_replacements(pfac_ctx *ctx, const uint32_t *offsets, uint64_t n_states, const void *bytes, uint64_t n_bytes);
/* Rewrites the slot's last scan with its last leftmost-longest selection (picks (p_k, s_k), made from `entry`, ending in
 * `exit`; L_k = the final length of s_k, R_k = its replacement):
 *   input[entry : p_0] + R_0 + input[p_0 + L_0 : p_1] + R_1 + ... + R_{n-1} + input[p_{n-1} + L_{n-1} : n_owned]
 * (a slice with end <= start is empty; no picks: input[entry : n_owned]).  *out_bytes = n_owned + exit - entry +
 * sum_k (R_k - L_k).  Chained ranges (entry = the previous range's exit) concatenate to the output of one scan of all.
 *   d_input  NULL = the slot's input buffer; else the buffer the scan read (16-B aligned)
 *   d_sel    NULL = the slot-owned selection; else the caller's d_out of pfac_records_leftmost_longest
 *   d_out    NULL = a slot-owned buffer grown to fit (fetched with pfac_replace_d2h); else a device pointer, 16-B aligned,
 *            of out_cap bytes.  No byte at or past *out_bytes is written.
 * Returns once *out_bytes is known; the writes are asynchronous on the slot's stream.  PFAC_E_OVERFLOW (with *out_bytes
 * exact, nothing written) when out_cap is too small for a caller's d_out.  PFAC_E_STATE without a selection since the
 * slot's last scan, for a selection made with an earlier table, or without replacements or final lengths for the current
 * table, or after a pfac_slot_reserve that replaced a buffer of the slot (no scan to rewrite).  PFAC_E_ARG for misaligned
 * buffers or a d_sel that is not the selection of this scan.
 * Kernels: a count pass sums R_k - L_k per 1024 picks (and per block of 64), the group prefix, then an output-driven
 * write: each wave finds the block of its first output byte by a 64-ary search over the block offsets, rebuilds the
 * block's segment offsets with a wave prefix and assembles 16 output bytes per lane in registers (one dwordx4 store;
 * only the last partial 16 B of the output is stored in pieces).  Input reads stay inside [0, n_avail) of the scan. */
int pfac_replace_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, void *d_out,
                                  uint64_t out_cap, uint64_t *out_bytes);
/* D2H of bytes [first, first + n) of the slot-owned output of the last pfac_replace_leftmost_longest.  Asynchronous on
 * the slot's stream; pfac_slot_sync completes it. */
int pfac_replace_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n);

/* Find-and-replace per document: pfac_replace_leftmost_longest over the slot's last selection, which must be a
 * pfac_records_leftmost_longest_documents since the slot's last scan (else PFAC_E_STATE).  The output is every
 * document's own output concatenated, with the same contract, arguments and errors as pfac_replace_leftmost_longest;
 * alongside it the output offsets out_off[n_docs + 1]: out[out_off[d] : out_off[d+1]] is document d's output,
 *   out_off[d] = off[d] + sum_{k < doc_first[d]} (R_k - L_k),   out_off[n_docs] = *out_bytes.
 *   d_doc_offsets  the offsets the selection cut with: NULL = the slot's (PFAC_E_STATE if the selection was given the
 *                  caller's, or if pfac_slot_doc_offsets replaced the slot's since); else the caller's device buffer
 *   d_doc_first    the selection's doc_first: NULL = its slot-owned one (PFAC_E_STATE if it went to the caller's
 *                  buffer); else that buffer
 *   d_out_offsets  NULL = a slot-owned buffer (fetched with pfac_replace_documents_d2h); else 8-B aligned, n_docs + 1
 * Extra kernels behind the write, O(n_picks + n_docs): one wave per block of 64 picks writes D_k = sum_{j<k} (R_j - L_j)
 * for every pick (8 B of scratch per pick), then one thread per document writes out_off[d] = off[d] + D_{doc_first[d]}.
 * The bytes are fetched with pfac_replace_d2h. */
int pfac_replace_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                           const uint64_t *d_doc_first, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets, uint64_t *out_bytes);
/* D2H of the slot-owned output offsets of the last pfac_replace_documents (n_docs + 1 entries).  Asynchronous on the
 * slot's stream; pfac_slot_sync completes it. */
int pfac_replace_documents_d2h(pfac_ctx *ctx, int slot, uint64_t *host_out_offsets);

/* Replacement templates: replacements that quote the matched text (sed's `&`, grep --color, <mark>...</mark>,
 * [ORG:...]).  offsets, bytes and n_bytes follow the contract, the limits and the errors of pfac_table_set_replacements;
 * splits holds one entry per final state:
 *   splits[s] == PFAC_TEMPLATE_PLAIN   a pick of state s is replaced by R_s, as pfac_table_set_replacements has it
 *   splits[s] <= R_s                   the pick (p, s) of length L is rewritten to
 *                                        R_s[:split] + input[p : p + L] + R_s[split:]
 *                                      with the input's bytes as the caller wrote them -- under a case fold
 *                                      (pfac_table_set_case_fold) the matcher saw folded bytes, the output carries the
 *                                      unfolded ones.  One quote of the whole match per template.
 *   any other value                    PFAC_E_ARG
 * splits == NULL: every state is plain, which is pfac_table_set_replacements; that call itself clears the splits.
 * Everything is checked before anything changes: a refused call leaves the earlier replacements and splits in force.
 * The splits are one more device attachment of the installed table: a table upload drops them with the replacements.
 * The old buffers are freed behind the device's queued work (a write kernel that still reads them has finished), as
 * the spans and the groups are.
 * With templates pfac_replace_leftmost_longest and pfac_replace_documents keep their signatures and contracts:
 *   *out_bytes = n_owned + exit - entry + sum_k (R_k - L_k * [state s_k is plain]),
 * out_off[d] of the documents call follows the same per-pick delta, chained ranges still concatenate (a pick that
 * starts below n_owned and ends in the halo is emitted whole by the range that owns its start), and input reads stay
 * inside [0, n_avail).  While no state quotes, the replaces run the kernels they ran before this call existed. */
#define PFAC_TEMPLATE_PLAIN 0xFFFFFFFFu
int pfac_table_set_replacement_templates(pfac_ctx *ctx, const uint32_t *offsets, const uint32_t *splits,
                                         uint64_t n_states, const void *bytes, uint64_t n_bytes);

/* Match extraction (grep -o): the rewritten picks of the slot's last leftmost-longest selection alone, back to back,
 *   E_0 + E_1 + ... + E_{n-1},   E_k = R_k[:split] + input[p_k : p_k + L_k] + R_k[split:]   (a plain state: R_k alone)
 * with no gaps between them and no tail behind them.  With the template (b"", b"\n") on every state this is what
 * grep -o prints.
 *   d_input, d_sel   as pfac_replace_leftmost_longest; the selection may be the whole-stream one or the per-document one
 *                    (document d's matches are out[pick_off[doc_first[d]] : pick_off[doc_first[d + 1]]])
 *   d_out            NULL = a slot-owned buffer OF THE EXTRACTION's own (fetched with pfac_extract_d2h): a later replace
 *                    does not invalidate it, nor does an extraction invalidate the replace's; else a device pointer,
 *                    16-B aligned, of out_cap bytes.  No byte at or past *out_bytes is written.
 *   d_pick_offsets   pick_off[k] = the output offset of E_k, pick_off[n] = *out_bytes: n + 1 entries (n = the
 *                    selection's count), 8-B aligned; NULL = a slot-owned buffer (pfac_extract_offsets_d2h)
 * *out_bytes = sum_k |E_k|; no picks: zero bytes and pick_off[0] = 0.  Preconditions, argument checks, PFAC_E_OVERFLOW
 * (with *out_bytes exact, nothing written -- the pick offsets neither) and PFAC_E_STATE are those of
 * pfac_replace_leftmost_longest, in its order.  Chained ranges concatenate; the caller rebases the offsets by the
 * bytes of the ranges before.
 * Kernels: the replace's three with every gap taken as empty and no tail segment -- the count pass sums |E_k|, the
 * write is the same output-driven one, and the per-pick prefix kernel of pfac_replace_documents writes the offsets. */
int pfac_extract_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel,
                                  void *d_out, uint64_t out_cap, uint64_t *d_pick_offsets, uint64_t *out_bytes);
/* D2H of bytes [first, first + n) of the slot-owned output of the last pfac_extract_leftmost_longest.  Asynchronous on
 * the slot's stream; pfac_slot_sync completes it. */
int pfac_extract_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n);
/* D2H of the slot-owned pick offsets of the last pfac_extract_leftmost_longest (n + 1 entries).  Asynchronous on the
 * slot's stream; pfac_slot_sync completes it. */
int pfac_extract_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_pick_offsets);

/* Tokenization: the token ids of the leftmost-longest picks, in order -- greedy longest-match (forward maximum
 * matching, the MaxMatch step of WordPiece, a dictionary tokenizer) with a per-byte fallback.  Two attachments of the
 * installed table: tok[s], an int32 per final state, and btok[b], an int32 per byte value; PFAC_TOKEN_DROP is allowed
 * in both.  state_ids holds n_states == num_final entries (else PFAC_E_ARG), byte_ids 256 (NULL = every byte DROP);
 * every value must be >= 0 or PFAC_TOKEN_DROP (else PFAC_E_ARG).  A pattern id's token goes to its state as a
 * replacement does.  Everything is checked before anything changes.  A device attachment like the replacements: a
 * table upload drops it, and the old buffers are freed behind the device's queued work. */
#define PFAC_TOKEN_DROP (-1)
int pfac_table_set_token_ids(pfac_ctx *ctx, const int32_t *state_ids, uint64_t n_states, const int32_t *byte_ids);
/* THE RULE.  Over the slot's last finished scan (n_owned, n_avail, its input) and its last leftmost-longest selection
 * (picks (p_k, s_k), k < n, ascending, made from `entry`, ending in `exit`; L_k = the final length of s_k), with C the
 * union of [p_k, p_k + L_k): every position i of [entry, n_owned), ascending,
 *   - if i == p_k for some k: emits tok[s_k], unless that is PFAC_TOKEN_DROP;
 *   - else if i is not in C: emits btok[input[i]], unless that is PFAC_TOKEN_DROP;
 *   - else emits nothing.
 * input[i] is the byte as the caller wrote it: under a case fold (pfac_table_set_case_fold) the matcher saw folded
 * bytes, btok sees the unfolded ones.  Every position emits at most one token.  *n_tokens is their number, ids[j] the j-th token and, with
 * PFAC_TOKENS_POSITIONS, pos[j] its position i as uint32, relative to the scan (like pfac_record.pos).  No position at
 * or past n_owned emits; a pick that starts below n_owned and ends in the halo emits its one token, and the next
 * range's entry skips its bytes: chained ranges (entry = the previous range's exit) concatenate to the tokens of one
 * scan of the whole range (positions: plus each range's base).
 *   d_input  NULL = the slot's input buffer; else the buffer the scan read (16-B aligned)
 *   d_sel    NULL = the slot-owned selection; else the caller's d_out of the selection (8-B aligned).  Checked on the
 *            device in the count pass: states below num_final, picks ascending and not overlapping, none before entry
 *            or at or past n_owned, the last end agreeing with exit.
 *   d_ids    NULL = a slot-owned buffer of this pass's own (fetched with pfac_tokens_d2h): no replace, extraction or
 *            other pass invalidates it, and it invalidates none; else 16-B aligned, holding out_cap entries
 *   d_pos    without PFAC_TOKENS_POSITIONS it must be NULL; with it NULL = slot-owned, else 16-B aligned, out_cap entries
 * No word at or past *n_tokens is written (the output is not rounded up to 16 bytes).  Input reads stay inside
 * [0, n_avail).  Returns once *n_tokens is known (one copy back per call); the writes are asynchronous on the slot's
 * stream.  PFAC_E_STATE (checked first, in the order of pfac_replace_leftmost_longest): no selection since the slot's
 * last scan, a selection of an earlier table, no token ids or no final lengths for the current table, a
 * pfac_slot_reserve that replaced a buffer.  PFAC_E_ARG: unknown flags, d_pos without the flag, misaligned buffers, a
 * d_sel that is not a selection of this scan and table.  PFAC_E_OVERFLOW (with *n_tokens exact, nothing written to any
 * buffer of the call) when out_cap is too small for a caller's d_ids or d_pos.
 * Kernels (position-driven over the scan's 4 KiB tiles; the replace's pick-driven passes do not fit, because with DROP
 * in btok the tokens of a gap depend on its bytes and a gap has no length bound): one thread per tile finds the tile's
 * first pick; a count pass builds every tile's 4096-bit "emits" bitmap in LDS (coverage and kept pick starts from the
 * tile's picks, btok from LDS for the bytes) and keeps it with a 16-bit token prefix per 64-bit word and the sums per
 * 64 tiles; the group prefix; then a write pass that ranks every token by popcounts of the saved bitmap, stages the
 * tile's tokens in LDS in rank order and stores whole 16-B chunks, the ragged ends in pieces. */
#define PFAC_TOKENS_POSITIONS 1u
int pfac_tokenize_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                                   int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens);
/* Tokenization per document: pfac_tokenize_leftmost_longest over the slot's last selection, which must be a
 * pfac_records_leftmost_longest_documents since the slot's last scan (else PFAC_E_STATE), with the same ids, plus
 * tok_off[n_docs + 1]: tok_off[d] = the tokens at positions < off[d], tok_off[n_docs] = *n_tokens.  No pick crosses a
 * document end, so ids[tok_off[d] : tok_off[d + 1]] is what tokenizing document d alone gives; ids and tok_off are the
 * pair that torch.nn.functional.embedding_bag(input, weight, offsets) takes (offsets = tok_off[:-1]).
 *   d_doc_offsets, d_doc_first   as pfac_replace_documents, with its NULL rules and PFAC_E_STATE cases
 *   d_tok_offsets                NULL = a slot-owned buffer (pfac_tokens_offsets_d2h); else 8-B aligned, n_docs + 1
 * One more kernel: a thread per document, tok_off[d] = group prefix + tile prefix + word prefix + a popcount. */
int pfac_tokenize_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                            const uint64_t *d_doc_first, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                            uint64_t *d_tok_offsets, uint64_t *n_tokens);
/* D2H of tokens [first, first + n) of the slot-owned result of the last tokenize pass (host_pos may be NULL; else the
 * pass must have written slot-owned positions).  Asynchronous on the slot's stream; pfac_slot_sync completes it. */
int pfac_tokens_d2h(pfac_ctx *ctx, int slot, int32_t *host_ids, uint32_t *host_pos, uint64_t first, uint64_t n);
/* D2H of the slot-owned token offsets of the last pfac_tokenize_documents (n_docs + 1 entries). */
int pfac_tokens_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_tok_off);

/* WordPiece: `##` continuation pieces and one [UNK] per word, over the passes above.  Whether a piece is word-initial
 * depends on the input alone, and WordPiece never backtracks (the longest admissible piece, and a word with an
 * untokenizable remainder is one [UNK]); so it is (1) the scan's records without those whose pattern is not in the
 * vocabulary half their position asks for, (2) the leftmost-longest selection, (3) every word the picks do not cover
 * completely collapsed into one [UNK].  ONE automaton over the stripped strings (`##ing` is inserted as `ing`); every
 * final state has two ids.
 * The attachment of the installed table: first_ids[s] / cont_ids[s], int32[n_states == num_final] each (kept on the
 * device as one 8-byte pair per state), the id of s at a word's start / inside a word; byte_ids int32[256] (NULL =
 * every byte DROP); every value >= 0 or PFAC_TOKEN_DROP.  unk_id >= 0.  word_set: the 256 bits of
 * pfac_records_filter_words (NULL = [0-9A-Za-z_]).  max_word_bytes in 1..4095 (BERT's default is 100 characters; this
 * cap counts bytes): a good word therefore touches at most two 4 KiB tiles, and a tile of word bytes alone holds a bad
 * word by itself.  PFAC_E_ARG for anything else, PFAC_E_STATE before an upload; everything is checked before anything
 * changes.  A table upload drops the attachment; it does not touch the ids of pfac_table_set_token_ids. */
int pfac_table_set_wordpiece(pfac_ctx *ctx, const int32_t *first_ids, const int32_t *cont_ids, uint64_t n_states,
                             const int32_t *byte_ids, int32_t unk_id, const uint64_t word_set[4], uint32_t max_word_bytes);
/* Role filter: the third sibling of pfac_records_filter_words and pfac_records_filter_spans.  With W the attachment's
 * word set, role(p) = FIRST if p == 0 or in[p - 1] is not in W, else CONT.  A record (p, s) stays iff in[p] is in W
 * and the id of role(p) for s is not PFAC_TOKEN_DROP.  As the other filters: heap, tile index and count are rewritten
 * IN PLACE; every reader and pass sees the kept records afterwards; a selection made before is stale; filters compose;
 * an error leaves everything untouched.  d_input / d_records as pfac_records_filter_words.  PFAC_E_STATE (first, in
 * the order of pfac_records_filter_spans): no finished scan, no final lengths, an earlier table, no WordPiece
 * attachment, an overflowed heap.  The slot remembers that its scan went through this filter and under which
 * attachment.  No documents form: where document offsets are word boundaries the byte rule already makes a document's
 * first byte FIRST. */
int pfac_records_filter_roles(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, uint64_t *n_kept);
/* THE RULE.  Over the slot's last finished scan and its last leftmost-longest selection (picks (p_k, s_k), made from
 * entry 0), with C the union of the picks' byte ranges: a WORD is a maximal run of bytes of W inside [0, n_owned)
 * (position n_owned ends a word); it is GOOD iff it is at most max_word_bytes long and every byte of it lies in C.
 * Every position i of [0, n_owned), ascending:
 *   - the first byte of a bad word emits unk_id; nothing else in that word emits;
 *   - a pick start p_k inside a good word emits the role(p_k) id of s_k, unless that is PFAC_TOKEN_DROP;
 *   - a byte not in W and outside C emits byte_ids[input[i]] (the byte as the caller wrote it, whatever the case
 *     fold), unless that is PFAC_TOKEN_DROP;
 *   - a byte not in W inside C emits nothing.
 * The rule is stated on bitmaps and stays defined when a pattern holds a byte outside W; it only stops being BERT's.
 * Parameters, PFAC_TOKENS_POSITIONS, the outputs (the slot-owned ones are the tokenizer's own: ONE result shared with
 * pfac_tokenize_*, fetched with pfac_tokens_d2h / pfac_tokens_offsets_d2h), PFAC_E_OVERFLOW (exact *n_tokens, nothing
 * written), the device checks of d_sel and the one copy back per call are those of pfac_tokenize_leftmost_longest and
 * pfac_tokenize_documents.  PFAC_E_STATE, before PFAC_E_ARG: every state of those calls (with the WordPiece attachment
 * in the place of the token ids); then a scan that has not been through pfac_records_filter_roles under the current
 * attachment; then a selection made from entry != 0.  The documents form also needs every document offset on a word
 * boundary -- off[d] is 0 or n_owned, or one of in[off[d] - 1], in[off[d]] is not in W (lines cut at a delimiter
 * outside W are) -- checked on the device, one thread per offset; else PFAC_E_ARG, nothing written.
 * Chained ranges (an entry, a word across n_owned) are out of scope: cut chunks at a byte outside W.
 * Kernels: the tokenizer's first-pick search, group prefix and document offsets unchanged; an edge pass (a wave per
 * tile: the bitmaps of word bytes, uncovered word bytes, kept pick starts and byte emitters, kept for the next pass,
 * and an 8-byte summary of the runs on the tile's two edges); a count pass that reads the two neighbours' summaries
 * and floods "bad" along the runs of word bits in registers; a write pass like the tokenizer's. */
int pfac_wordpiece_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                                    int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens);
int pfac_wordpiece_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                             const uint64_t *d_doc_first, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                             uint64_t *d_tok_offsets, uint64_t *n_tokens);

/* Unigram (the SentencePiece family: T5, ALBERT, XLNet, mBART): every piece has a score, a word is cut into the
 * pieces with the highest total, by Viterbi over the lattice of ALL vocabulary matches inside the word -- which is what
 * the record heap of a scan holds, in (position, length) order.  The first token pass over the heap itself, not over a
 * selection.  ONE automaton over the stripped strings, as for WordPiece (`▁the` is inserted as `the` and goes to the
 * FIRST half of its state, a plain `the` to the CONT half).
 * The attachment of the installed table: pieces[s], one 16-byte entry per final state (n_states == num_final); ids
 * >= 0 or PFAC_TOKEN_DROP; byte_ids int32[256] (NULL = every byte DROP); byte_score, the score of a byte edge; unk_id
 * >= 0 (a run of byte edges is one unk_id) or PFAC_TOKEN_DROP (byte fallback: every byte edge emits its byte id);
 * word_set as for WordPiece, but NULL = every byte except \t \n \v \f \r and space (SentencePiece splits at
 * whitespace); max_word_bytes in 1..4095.  Scores are integers, the caller's log-probabilities in fixed point; sums
 * stay in int32: every score, byte_score included, must satisfy |score| * (max_word_bytes + 1) < 2^31.  PFAC_E_ARG for
 * anything else, PFAC_E_STATE before an upload; everything is checked before anything changes.  A table upload drops
 * the attachment; old buffers are freed behind queued work; a slot-owned result made under an earlier attachment is
 * stale (PFAC_E_STATE from the fetches).  It touches neither the token ids nor the WordPiece attachment. */
typedef struct pfac_unigram_piece { int32_t first_id, cont_id, first_score, cont_score; } pfac_unigram_piece;
int pfac_table_set_unigram(pfac_ctx *ctx, const pfac_unigram_piece *pieces, uint64_t n_states, const int32_t *byte_ids,
                           int32_t byte_score, int32_t unk_id, const uint64_t word_set[4], uint32_t max_word_bytes);
/* THE RULE.  Over the slot's last finished scan: n_owned, n_avail, its input, and its records as they stand (filtered
 * or not).  W is the word set, L_s the final length of state s.  A WORD is a maximal run of bytes of W inside
 * [0, n_owned) (position n_owned ends a word).  For a word [a, b), n = b - a, the nodes are 0..n and
 *   - PIECE EDGES: if n <= max_word_bytes, every record (p, s) with a <= p and p + L_s <= b is an edge
 *     p - a -> p - a + L_s carrying (first_id, first_score) of s when p == a, (cont_id, cont_score) otherwise; the edge
 *     exists only if that id is not PFAC_TOKEN_DROP.  A word longer than the cap has no piece edges;
 *   - BYTE EDGES: j -> j + 1 with byte_score, always;
 *   - best[0] = 0, best[j] = the maximum over the edges i -> j of best[i] + score; of equal candidates the smaller i
 *     wins (the longer edge), and of a one-byte piece and the byte edge the piece;
 *   - the path is the backtrack from n: it is unique.
 * Every position of [0, n_owned) emits at most one token, ascending:
 *   - a piece edge of a path emits its id at its first byte;
 *   - with unk_id >= 0, every maximal run of consecutive byte edges on one word's path emits one unk_id at the run's
 *     first byte; with unk_id == PFAC_TOKEN_DROP every byte edge emits byte_ids[in[i]], unless that is DROP;
 *   - a byte outside W emits byte_ids[in[i]], unless that is DROP (never unk_id);
 *   - in[i] is the byte as the caller wrote it, whatever the case fold.
 * d_input / d_records as pfac_records_filter_roles (NULL = the slot's buffers).  flags: PFAC_TOKENS_POSITIONS.  The
 * outputs, their NULL rules and alignments, PFAC_E_OVERFLOW (exact *n_tokens, nothing written) and the one copy back
 * per call are those of pfac_tokenize_*; the slot-owned result is the tokenizer's own ONE shared result
 * (pfac_tokens_d2h, pfac_tokens_offsets_d2h).  No word at or past *n_tokens is written; input reads stay below n_avail.
 * PFAC_E_STATE first, in the filters' order: no finished scan, no final lengths, a scan of an earlier table, no
 * Unigram attachment for the current table, an overflowed heap, a reserve that replaced a slot buffer the call would
 * use.  Then PFAC_E_ARG: unknown flags, d_pos without the flag, a d_records that is not the scan's heap, misalignment.
 * The documents form needs offsets that start at 0, do not decrease and end at n_owned, each on a word boundary
 * (WordPiece's rule, checked on the device, one thread per offset); else PFAC_E_ARG and nothing written.  tok_off is
 * as in pfac_tokenize_documents.  Chained ranges are out of scope: cut chunks at a byte outside W.
 * Kernels: a solve pass (a workgroup per 4 KiB tile; the tile's words and the one that enters from the left, one lane
 * per word: forward DP in LDS in heap order, backtrack into the bitmaps "edge start" and "byte edge", kept per tile
 * with the emit bitmap and its prefixes); the tokenizer's group prefix and document offsets; a write pass like the
 * tokenizer's that finds a piece's state as the record (p, L).  Measured: 24.8 ms for 1 GiB of text with
 * 448.7 M records, 1.06 times the role filter + selection + WordPiece pass over the same buffer. */
int pfac_unigram_records(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, uint32_t flags, int32_t *d_ids,
                         uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens);
int pfac_unigram_documents(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, const uint64_t *d_doc_offsets,
                           uint64_t n_docs, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                           uint64_t *d_tok_offsets, uint64_t *n_tokens);

/* Byte-level BPE (GPT-2, RoBERTa, Llama 3, every tiktoken vocabulary): a word starts as its single bytes and the
 * adjacent pair whose concatenation has the lowest merge rank is merged, until no pair has one.  "Is the concatenation
 * of these two parts a vocabulary string, and which merge makes it" is a lookup of (start, length) among the records of
 * the word: the second token pass over the record heap itself, with no pair table and no second automaton.  The
 * automaton holds the vocabulary strings of at least 2 bytes that a merge makes; single-byte tokens go to byte_ids.
 * The attachment of the installed table: pieces[s], one 16-byte entry per final state (n_states == num_final): id >= 0
 * or PFAC_TOKEN_DROP; rank >= 0, the index of the merge that makes this string; split, the byte length of that merge's
 * left half, or 0 for "any split" (tiktoken's form, where the rank belongs to the string; a split >= L_s can never
 * apply and is not an error); reserved 0.  byte_ids int32[256] (NULL = every byte DROP); word_set as for Unigram (NULL =
 * every byte except \t \n \v \f \r and space); lead, a byte value 0..255 that is not in the word set, or -1 for none;
 * max_word_bytes in 1..255.  PFAC_E_ARG for anything else, PFAC_E_STATE before an upload; everything is checked before
 * anything changes.  The lifetime is the Unigram attachment's: a table upload drops it; a new one is installed whole
 * behind queued work; a slot-owned result made under an earlier attachment is stale (PFAC_E_STATE from the fetches).  It
 * touches none of the other three attachments (token ids, WordPiece, Unigram). */
typedef struct pfac_bpe_piece { int32_t id, rank; uint32_t split, reserved; } pfac_bpe_piece;
int pfac_table_set_bpe(pfac_ctx *ctx, const pfac_bpe_piece *pieces, uint64_t n_states, const int32_t *byte_ids,
                       const uint64_t word_set[4], int32_t lead, uint32_t max_word_bytes);
/* THE RULE.  Over the slot's last finished scan: n_owned, n_avail, its input, and its records as they stand (filtered
 * or not).  W is the word set, L_s the final length of state s.
 * WORDS.  A RUN is a maximal run of bytes of W inside [0, n_owned).  The WORD of a run [a, b) is [a - 1, b) if
 * lead >= 0, a > 0 and in[a - 1] == lead, else [a, b): of several lead bytes in a row only the last belongs to the word
 * (what GPT-2's pre-tokenizer does with spaces).
 * MERGES.  For a word [a, b) with n = b - a <= max_word_bytes:
 *   - the parts start as the n single bytes;
 *   - two adjacent parts [l, k), [k, r) are a CANDIDATE iff the heap holds a record (l, s) with L_s == r - l, and
 *     pieces[s].split is 0 or k - l; the candidate's rank is pieces[s].rank;
 *   - the candidate with the lowest rank is merged; among equal ranks the smallest l wins;
 *   - repeat until there is no candidate.
 * A word longer than the cap has no candidates: its parts stay single bytes.
 * EMISSION.  Every position of [0, n_owned) emits at most one token, ascending:
 *   - a part of two or more bytes emits pieces[s].id of its record (l, s) at l, unless that is PFAC_TOKEN_DROP;
 *   - a part of one byte, and every byte outside all words, emits byte_ids[in[i]], unless that is DROP;
 *   - in[i] is the byte as the caller wrote it, whatever the case fold.
 * With split set this is the merge-list rule of the usual BPE implementations as long as no two merges make the same
 * string: the left part equals the merge's left half iff the concatenation matches and the split point agrees.
 * d_input / d_records, flags (PFAC_TOKENS_POSITIONS), the outputs, their NULL rules and alignments, PFAC_E_OVERFLOW
 * (exact *n_tokens, nothing written), the one copy back per call and the ONE slot-owned token result (pfac_tokens_d2h,
 * pfac_tokens_offsets_d2h) are those of pfac_unigram_records / pfac_unigram_documents.  No word at or past *n_tokens is
 * written; input reads stay below n_avail.  PFAC_E_STATE first, in the filters' order: no finished scan, no final
 * lengths, a scan of an earlier table, no BPE attachment for the current table, an overflowed heap, a reserve that
 * replaced a slot buffer the call would use.  Then PFAC_E_ARG: unknown flags, d_pos without the flag, a d_records that is
 * not the scan's heap, misalignment.  The documents form needs offsets that start at 0, do not decrease and end at
 * n_owned; none may lie strictly inside a word, and the position between a lead byte and its run counts as inside
 * (checked on the device, one thread per offset); else PFAC_E_ARG and nothing written.  Chained ranges are out of scope:
 * cut chunks at a byte outside W that is not a lead.
 * Kernels: a solve pass (a workgroup per 4 KiB tile and 256 bytes on either side, one lane per word: a
 * first-record index per position and a cached rank per boundary in LDS, the lowest rank merged until none is left), the
 * tokenizer's group prefix and document offsets, a write pass that finds a part's id as the record (p, L).  Measured
 * (DESIGN.md 29): 81.4 ms for 1 GiB of text with 948.2 M records under 194 merges, 2.34 times the Unigram pass over
 * the same records. */
int pfac_bpe_records(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, uint32_t flags, int32_t *d_ids,
                     uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens);
int pfac_bpe_documents(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, const uint64_t *d_doc_offsets,
                       uint64_t n_docs, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                       uint64_t *d_tok_offsets, uint64_t *n_tokens);

/* Synthetic input generators, written straight into device memory (the
 * reference built big inputs by tiling a small text, creatbiginput.sh:2-5).
 *   tiled : byte i = pattern[(phase + i) % period]
 *   random: byte i = byte (i&7) of splitmix64(seed + (i>>3))  (counter based) */
int pfac_fill_tiled(pfac_ctx *ctx, int slot, void *d_dst, uint64_t n, const void *host_pattern, uint32_t period,
                    uint64_t phase);
int pfac_fill_random(pfac_ctx *ctx, int slot, void *d_dst, uint64_t n, uint64_t seed);

/* Kernel introspection for bench/DESIGN: variant chosen for the uploaded table
 * (0 = tables in LDS, 1 = tables via L2), tile bytes, grid size, LDS bytes. */
int pfac_scan_info(pfac_ctx *ctx, int *variant, int *tile_bytes, int *grid_blocks, int *lds_bytes);
/* ... and the staging layout the NEXT scan will use: buffers per wave (3 / 2: a tile's records leave two / one
 * round(s) after it was scanned; 1: dense mode, emitted at once) and records per buffer (a tile with more is
 * walked a second time; 4096 = dense mode's second form, where it is the wave's record log in device memory that
 * bounds a tile).  The layout follows the match density of the scans before. */
int pfac_scan_staging(pfac_ctx *ctx, int *buffers, uint32_t *records_per_buffer);

/* ------------------------------------------------------------------ */
/* Drop-in shaped like the reference seam (main.cc:19-37).             */

/* Field-for-field struct thread_data (main.cc:19-32). */
typedef struct pfac_thread_data {
    unsigned char *input_string;
    int input_size;
    int state_num;
    int final_state_num;
    unsigned int *match_result;     /* dense: input_size * max_pat_len slots, 0xFFFFFFFF = empty */
    int HTSize;
    int width;
    int *s0Table;
    int max_pat_len;
    int *r;
    int *HT;
    int *val;
} pfac_thread_data;

/* GPU_Malloc_Memory + GPU_TraceTable + GPU_Free_memory in one synchronous
 * call (master_kernel.cu:188-524): uploads dataset's tables and input to
 * `device`, scans, and fills dataset->match_result in the reference's dense
 * layout (slot j of position i = j-th final state reached from i, rest
 * 0xFFFFFFFF) so that main.cc:304-350 can run unchanged on it. */
int pfac_trace_table_compat(const pfac_thread_data *dataset, int device);

#ifdef __cplusplus
}
#endif
#endif /* PFAC_H */
