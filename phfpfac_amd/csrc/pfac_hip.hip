/*
 * pfac_hip.hip -- the MI355X (gfx950 / CDNA4) PFAC scan: kernels + C-ABI runtime.
 *
 * Replaces master_kernel.cu of the reference (TraceTable_kernel :92-180,
 * SUBSEG_MATCH :37-74, GPU_Malloc_Memory :188-257, GPU_TraceTable :277-455,
 * GPU_Free_memory :457-524).  Written for 64-wide wavefronts; not a
 * translation: the reference gives every offset a dense max_pat_len-slot
 * result row (4*max_pat_len bytes of HBM traffic per input byte, three times
 * over); this kernel emits compact, globally ORDERED records in a single pass
 * over the input: one 32-bit word  pos_in_tile:12 | final_state:20  per match
 * plus one 64-bit first-record index per 4 KiB tile (automata with more than
 * 2^20 final states fall back to 8-byte {pos, state} records).
 *
 * Kernel structure (one persistent workgroup per CU = up to 15 compute waves + 1 coordinator wave;
 * the unit of work is a WAVE TILE, 4 KiB of input owned by one wavefront; no workgroup barrier in the loop):
 *   ticket   the coordinator takes one BATCH of tiles (one per compute wave) per round with a single
 *            global atomic, three rounds ahead (four interleaved ticket counters)
 *   stage    each wave loads its 4 KiB with 16-B-per-lane buffer loads (hardware bounds check ->
 *            bytes past n_avail read as 0), one round ahead, and mirrors them + the max_pat_len-1
 *            halo into its private LDS region
 *   root     32-bit "has a root edge" mask per lane per 32 contiguous bytes (two halves per tile): SWAR
 *            compare + v_dot4 when the root has a single edge, else one LDS flag lookup per byte (mk.cu:41)
 *   level 2  most walks die on their second byte, so survivors are classified before any walk: DEEP when the
 *            byte pair starts a path of length 2 in the trie (bit-parallel SWAR compare for a single-edge root
 *            with <= 2 grandchildren, else one lookup per survivor in a 2-byte-prefix bitmap in LDS), SHALLOW-FINAL
 *            when they are not deep but the depth-1 state is final (exactly one record, known without a walk);
 *            everything else is dropped on the spot
 *   compact  DPP prefix sums append the kept survivors' positions, in order, to a FIFO in LDS; a tile without deep
 *            survivors writes its records straight to the staging buffer instead (no FIFO, no walk)
 *   walk     rounds of 64 (x NWALK) FIFO entries; straight-line, predicated: root row and the dense depth-1 rows
 *            from LDS, deeper states through the perfect hash  state = PHF(state, byte)  from LDS (small tables)
 *            or L2 (large: 2-4 walks per lane, slots fused with the next state's r[] so a step is one gather);
 *            final states are recorded as they are met (mk.cu:49-71); a round without deep entries skips the walk
 *   stage    records (pos:12 | state:20) go to an LDS staging buffer in (position, length) order
 *   place    per-wave counts -> coordinator, which places the round's tiles back to back in the workgroup's current
 *            CHUNK of the record heap (one atomic on the heap cursor per chunk, the next chunk always on order: no
 *            workgroup ever waits for another), writes every wave's first record index back to LDS and the tiles'
 *            index words (first record | count << 40) to memory -- all in the round the counts came in
 *   emit     one round later the wave copies its staged words to the heap, 16 B per lane.  Walking the tile index
 *            in order gives the records sorted by (position, pattern length), the reference's output order
 *            (main.cc:341-349).  Tiles with more records than the staging buffer holds are re-walked writing
 *            straight to the heap; "dense mode" (one big staging buffer, synchronous emission) takes over when most
 *            tiles are like that.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <type_traits>
#include <string>
#include <vector>

#include "pfac.h"
#include "pfac_fold.h"

namespace {

// ---------------------------------------------------------------------------
// geometry.  The unit of work is a WAVE TILE: 4 KiB of input owned by one wavefront.
constexpr int WAVE = 64;
constexpr int SUB = WAVE * 16;             // bytes one wave covers with one 16-B-per-lane load (1 KiB)
constexpr int SUBS = 4;                    // such sub-tiles per wave tile
constexpr int WTILE = SUB * SUBS;          // 4096: tile-local positions fit 12 bits
constexpr int MSUBS = 2;                   // root test / compaction: the tile as 2 halves, a lane owning 32 contiguous bytes of each
constexpr int MSUB = WTILE / MSUBS;        // 2048
constexpr int MLANE = MSUB / WAVE;         // 32 bytes per lane -> one 32-bit survivor mask
constexpr int HALO_MAX = 1024;             // >= max_pat_len - 1 (patterns are < 1024 bytes), multiple of 16
constexpr int QCAP = SUB / 2 + 4 * WAVE;   // survivor FIFO: < one round (at most 4 x 64) carried over + up to 512 appended at a time
#ifndef PFAC_CAPW
#define PFAC_CAPW 256
#endif
constexpr int CAPW = PFAC_CAPW;            // records staged in LDS per tile per buffer (more -> synchronous re-walk)
static_assert(CAPW % 8 == 0, "staging buffers start on 16-byte boundaries (copy_out reads them 16 bytes per lane)");
constexpr int PACK_STATE_BITS = 20;        // staged record = pos:12 | state:20 (larger automata re-walk)
constexpr int MAX_WAVES_PER_BLOCK = 16;     // 15 compute waves + the coordinator
constexpr int LDS_TOTAL = 160 * 1024;
constexpr int LDS_TABLE_MAX = 40 * 1024;   // PHF tables up to this size are staged in LDS (variant 0)

// shared (per workgroup) LDS: root row, 4 pre-shifted byte-wide flag tables (root-edge flag << k | can-be-a-second-byte
// flag << (k + 4), one table per byte of a dword), then the PHF tables (variant 0)
constexpr int SH_HDR = 0;                  // round rings (H_* below)
constexpr int SH_S0 = SH_HDR + 2048;
constexpr int SH_FTAB = SH_S0 + 256 * 4;
constexpr int SH_D1IDX = SH_FTAB + 4 * 256;  // 256 x u8: dense-row index of the depth-1 state reached on each root byte
constexpr int SH_FIN = SH_D1IDX + 256;     // 256 x u8: 1 where the depth-1 state reached on that root byte is final
constexpr int SH_COLMAP = SH_FIN + 256;    // 256 x u8: column of the dense rows a second byte maps to (the last column = no edge)
constexpr int SH_D1 = SH_COLMAP + 256;     // d1_rows dense rows int32[d1_stride] (the hot first-level transition rows), only the
                                           // columns of bytes that ARE the second byte of some pattern + one "no edge" column
constexpr int D1_LDS_MAX = 32 * 1024;      // the depth-1 states get dense rows when rows x columns x 4 B fit this (else none do)
constexpr int D1_STATE_BITS = 20;          // packed dense-row entry (FUSED): state | index of its r[] << 20
constexpr int D1_N2_MAX = 2048;            // ... so at most this many depth-2 states (the entry stays positive)
// the PHF tables (variant 0) follow the dense rows: SH_D1 + d1_lds_bytes; the 2-byte-prefix bitmap (bm2_rows x 32
// bytes) sits at ScanArgs::sh_bm2, behind them
#ifndef PFAC_L2F_UNROLL
#define PFAC_L2F_UNROLL 1
#endif
constexpr int L2F_UNROLL = PFAC_L2F_UNROLL;  // survivors classified per trip of the level-2 lookup loop
#ifndef PFAC_MASK_GATHERS
#define PFAC_MASK_GATHERS 1
#endif
constexpr bool MASK_GATHERS = PFAC_MASK_GATHERS != 0;   // fused walks: exec-mask the table gathers of dead walkers
#ifndef PFAC_LOAD_AUX
#define PFAC_LOAD_AUX 2
#endif
constexpr int LOAD_AUX = PFAC_LOAD_AUX;    // cache policy of the tile loads (0 default, 2 = nt: the input is read once)
#ifndef PFAC_PAIR_DENSITY_PCT
#define PFAC_PAIR_DENSITY_PCT 40              // level-2 filter: flags only (mode 3) from this share of (first, second) byte combinations on
#endif
constexpr int QDEEP = 0x8000;              // FIFO entry = tile-local position | QDEEP when the survivor needs a walk
// per-wave LDS: tile bytes + halo | survivor FIFO | nbuf record staging buffers.  A tile's records leave nbuf - 1 rounds
// after it was scanned (its record base needs every count of its round).  nbuf = 3 where LDS allows: the stores then
// go out at the TOP of a round, right behind the next tile's loads, and have the whole round to complete -- with two
// buffers they can only go at the END (the base of the previous round is not in earlier), and since loads and stores
// retire through one in-order counter (vmcnt) the next round's wait for its tile also waits for their write
// acknowledgements (measured: 6 % of the headline kernel).
constexpr int NBUF_MAX = 3;
constexpr int CAPW3_MIN = 192;             // the three-buffer layout needs room for this many records per buffer
constexpr int PW_FIXED_1BUF = WTILE + QCAP * 2;              // + nbuf * stage_cap * 4
// Dense mode (most tiles hold more matches than CAPW, e.g. a dictionary on text): ONE big staging buffer per
// wave and synchronous emission -- fewer waves fit, but a tile is walked once instead of twice.
constexpr int CAPW_DENSE = 2048;
constexpr int PW_FIXED_DENSE = PW_FIXED_1BUF + CAPW_DENSE * 4;
// Dense mode, second form (dense2_tile below: walker slots refilled the moment a walk ends, records logged out of order
// and put in order on their way out).  Per wave, behind the tile + halo: ring of pending walkers | match count of every
// tile position (4 bits each) | record prefix of every 8 positions (u16).
constexpr int D2_RING = 256;               // ring entries of 8 bytes (a power of two, >= 3 front-end batches of 64)
constexpr int D2_CNT_OFF = D2_RING * 8;
constexpr int D2_PREF_OFF = D2_CNT_OFF + WTILE / 2;
constexpr int D2_AUX = D2_PREF_OFF + (WTILE / 8) * 2;
static_assert(D2_AUX >= QCAP * 2 && D2_AUX % 16 == 0, "the survivor FIFO of the fallback pass lies in the same bytes");
constexpr int PW_FIXED_DENSE2 = WTILE + D2_AUX;              // (the record log is in device memory)
constexpr unsigned D2_LOG_CAP = 4096;     // words of log per wave (device memory; a tile with more records goes the classic way)

// Batch tickets: one address sustains ~85 M atomics/s, and at 4 TB/s with 60 KiB per ticket the workgroups ask for
// 65 M/s -- the single counter was the floor of the whole kernel (3.9 us per round with the scan compiled out).  So
// there are TICKET_WAYS counters, 256 bytes apart: workgroup j draws from counter j % ways and holds batches
// ticket * ways + j % ways.  Ids stay monotone per workgroup (it leaves when ITS counter runs past the end) and every
// batch below the end is drawn by somebody as long as every residue class has a workgroup (ways <= grid).  Nothing
// waits for a batch: a workgroup's record placement depends on no other workgroup (see "Record placement").
#ifndef PFAC_TICKET_WAYS
#define PFAC_TICKET_WAYS 4
#endif
constexpr unsigned TICKET_WAYS = PFAC_TICKET_WAYS;
constexpr unsigned CTL_WORDS = 64u * (TICKET_WAYS + 1);   // control header in 32-bit words: one 256-byte line per ticket counter + the cursor's
constexpr unsigned SPIN_MAX = 1u << 22;    // bounded spins (default; PFAC_SPIN_MAX): ~0.5 s of LDS polls, seconds of global polls
// words of the control header (first ticket line) the kernel reports through: device memory, ordinary device atomics
constexpr unsigned CTL_ERR = 32, CTL_OVF = 33, CTL_DONE = 34, CTL_OVF2 = 35, CTL_TOTAL = 36 /* u64: matches */;
constexpr unsigned CTL_T0 = 38;            // u64: ~(earliest entry time of the first T0_GROUPS workgroups), folded with a max (the header starts at zero)
constexpr unsigned T0_GROUPS = 8;          // (one workgroup per XCD: the dispatcher deals the first eight round-robin)
// words of the host-visible result block (ScanArgs::res, Slot::h_ctl) behind the counts
constexpr unsigned RES_DONE = 7;           // stored LAST by the last workgroup to leave, system-scope release: the scan's completion
constexpr unsigned RES_T0 = 16, RES_T1 = 18;       // u64 each: first workgroup in / last workgroup out, s_memrealtime ticks
constexpr unsigned CTL_CURSOR = 64u * TICKET_WAYS;     // u64: first free record of the heap (on a line of its own)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// the case fold of pfac_fold.h over the four dwords of a 16-byte load
__device__ __forceinline__ u32x4 fold4(u32x4 v) {
    u32x4 o;
    o[0] = pfac_fold_dword(v[0]); o[1] = pfac_fold_dword(v[1]); o[2] = pfac_fold_dword(v[2]); o[3] = pfac_fold_dword(v[3]);
    return o;
}

struct ScanArgs {
    const unsigned char *in;
    unsigned long long n_owned, n_avail;
    void *out;                            // the record heap: out_cap records of rec_bytes bytes
    unsigned long long out_cap;
    unsigned long long *tile_index;       // [n_tiles]: first record of the tile | its record count << 40
    unsigned chunk;                       // records a workgroup takes from the heap cursor at a time (0: exact allocations only)
    unsigned rec_bytes;                   // record form of this scan: 2 (pos:12 | state:4), 4 (pos:12 | state:20) or 8 (pfac_record)
    const int *s0;
    const int *r;
    const int2 *T;
    const int4 *T4;                       // FUSED: {owner row, next state, r[row of next state], 0} per slot (tables via L2)
    int r_words, t_entries;
    int ht_size, wbit, num_final, halo;   // halo: bytes readable past a tile, multiple of 16
    int rn_bias;                          // fused tables: T4 starts at slot -rn_bias (displacements may be negative); every index
                                          // the fused walk forms is slot + rn_bias >= 0
    int shared_bytes, pw_bytes;           // LDS carve: shared region, then one region per wave
    const int *d1;                        // dense rows of the depth-1 states, d1_rows x 256 (or null); in LDS: d1_rows x d1_stride
    const unsigned char *d1idx;           // root byte -> dense row index
    const unsigned char *d1_colmap;       // [256] second byte -> LDS column (d1_stride - 1: no pattern has it as second byte)
    const unsigned char *d1_colbyte;      // [d1_ncols] the byte of each LDS column
    int d1_rows;                          // 0: no dense level
    int d1_stride, d1_ncols, d1_lds_bytes;  // LDS row length in words (columns, + 1 "no edge" unless all 256 are used);
                                          // columns; bytes of the LDS rows (multiple of 16)
    const int2 *d1r2;                     // FUSED + packed dense rows: {r[], child mask} of the depth-2 states, d1_n2 entries (else null)
    int d1_n2;                            // > 0: a dense-row entry is  state | index into d1r2 << 20  (or -1)
    unsigned root_byte;                   // ROOT == 1: the only byte with a root edge, replicated x4
    int root_state;                       // ROOT == 1: the state that byte leads to (every survivor starts there)
    // level-2 filter (which survivors can go beyond their second byte):
    //   0 off: every survivor is walked        1 (ROOT == 1): SWAR compare with <= 2 child bytes of root_state
    //   2: one lookup per survivor in the 2-byte-prefix bitmap (bm2_rows = 256 rows of 32 bytes; ROOT == 1: its one row)
    //   3 (ROOT == 0, sec_filter): second-byte flags only -- survivors whose next byte can be a second byte are all walked
    int l2f_mode;
    unsigned child0, child1;              // mode 1: the child bytes, replicated x4 (n_child 1: child1 == child0)
    int n_child;                          // mode 1: 0 (nothing is ever deep), 1 or 2
    const unsigned char *bm2;             // mode 2: bit (b0 << 8 | b1) set iff a path b0 b1 leaves the root
    int bm2_rows, sh_bm2;                 // rows staged in LDS (256, or 1 = the root byte's row) at this LDS offset
    int sh_t0;                            // packed dense rows: LDS offset of the root table of dense2_tile (256 words), else 0
    const unsigned char *sec2;            // [256]: 1 where the byte is the second byte of some pattern (column OR of bm2)
    int sec_filter;                       // ROOT == 0, mode 2: pre-filter the lookups with sec2 (no 1-byte patterns)
    unsigned stage_cap;                   // records one staging buffer holds (0: final states do not fit the packed word)
    unsigned nbuf;                        // staging buffers per wave: 3 / 2 = emit two / one round(s) later, 1 = emit at once (dense mode)
    int dense2;                           // dense mode on fused tables with packed dense rows: the refilled-walker form (dense2_tile)
    unsigned *d2log;                      // ... its record logs: d2log_cap words per compute wave of the grid (device memory)
    unsigned d2log_cap;
    unsigned sparse_cap;                  // tiles with more matches than this are counted in res[3] (mode adaptation) ...
    unsigned small_cap;                   // ... and than this (the three-buffer capacity) in res[6]
    unsigned n_tiles;
    unsigned spin_max;             // bound of every spin loop
    unsigned fault;                // test knob (PFAC_FAULT): bit 0 = workgroup 1 never publishes the record bases of its second round
    unsigned *ctl;                 // control header (device memory): batch ticket counters 64 words apart; [CTL_ERR/OVF/DONE/TOTAL]:
                                   // error flags, tiles denser than sparse_cap, workgroups that have left, matches; [CTL_CURSOR]
    unsigned ticket_ways;          // counters in use: min(TICKET_WAYS, grid)
    uint4 *zero_next;              // the slot's OTHER control header: this launch zeroes it for the next one ...
    unsigned zero_vec;             // ... this many 16-byte units (no memset between back-to-back scans)
    unsigned *res;                 // host-mapped pinned words, no D2H copy, written with plain stores by the last workgroup
                                   // to leave: [0..1] matches (u64), [2] error flags, [3] tiles denser than sparse_cap,
                                   // [4..5] heap cursor = records of capacity used (u64), [6] tiles denser than small_cap,
                                   // [RES_T0], [RES_T1] the kernel's own start and end time -- and then [RES_DONE] = 1 with a
                                   // system-scope release: the host waits for THAT word, the dispatch carries no signal
    unsigned long long *dbg;       // PFAC_TRACE_BUILD only: per-round timestamps (10 ns units), else null
};

// ---------------------------------------------------------------------------
// wave helpers (wave = 64 lanes)

// Inclusive prefix sum over the 64 lanes with DPP (no LDS round trips): Hillis-Steele inside each
// row of 16 lanes (row_shr 1,2,4,8), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows
// 2 and 3.  Lanes without a source keep `old` = 0 (bound_ctrl off), i.e. add the identity.
__device__ __forceinline__ unsigned wave_incl_scan(unsigned x) {
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
    x += (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, WAVE);
    return x;
}
__device__ __forceinline__ unsigned bcast_last(unsigned x) { return __builtin_amdgcn_readlane(x, WAVE - 1); }
// LDS written by some lanes of a wave and read by others of the SAME wave:
// the LDS executes one wave's instructions in order; this keeps the compiler
// from moving accesses across and drains lgkmcnt.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup organisation.  A workgroup = NC compute waves + 1 coordinator wave, and proceeds in
// ROUNDS: in round r compute wave c scans tile  batch(r) * NC + c.  Batches are handed out in order by
// one global atomic per round (a ticket per 4 KiB tile would hit the ~88 M atomics/s an address
// sustains on MI355X and cap the scan at 0.36 TB/s), taken AHEAD rounds ahead by the coordinator.
// The coordinator also sums the round's per-wave match counts and places the round's tiles in the
// workgroup's chunk of the record heap, while the compute waves are already scanning the next round;
// they pick their first record index up from LDS when they emit, one round later.  No workgroup barrier
// in the loop, and no wait on any other workgroup: nothing depends on dispatch order, residency or
// placement (several grids of this kernel may run at once -- gphf's slots do).  The waits inside a
// workgroup (rings below) are bounded; a timeout ends the scan with PFAC_E_INTERNAL instead of hanging.
//
// LDS header (unsigned words), rings of 8 rounds indexed by r & 7:
constexpr int RING = 8;
#ifndef PFAC_AHEAD
#define PFAC_AHEAD 2
#endif
constexpr int AHEAD = PFAC_AHEAD;          // rounds the batch ring runs ahead of the coordinator's own round
static_assert(AHEAD >= 2 && AHEAD <= RING - 3, "ring depth");
#ifndef PFAC_LOAD_DEPTH
#define PFAC_LOAD_DEPTH 1
#endif
constexpr int LOAD_DEPTH = PFAC_LOAD_DEPTH; // tiles a compute wave keeps in flight ahead of the one it scans (1 or 2)
static_assert(LOAD_DEPTH == 1 || (LOAD_DEPTH == 2 && AHEAD >= 3), "two tiles in flight need the ring three rounds ahead");
constexpr int H_BATCH = 0;                 // batch id of round r
constexpr int H_EPOCH = 8;                 // == r + 1 once H_BATCH (and a zeroed H_ARRIVED) are valid
constexpr int H_ARRIVED = 16;              // compute waves that have posted their count
constexpr int H_READY = 24;                // == r + 1 once H_WBASE of round r is valid
constexpr int H_CNT = 48;                  // 16 words per round: match count of each compute wave
constexpr int H_WBASE = H_CNT + RING * 16; // 32 words per round: {lo, hi} first record index of each compute wave
constexpr int H_OVF = H_WBASE + RING * 32;  // tiles of this workgroup with more matches than sparse_cap
constexpr int H_EXIT = H_OVF + 1;          // waves of this workgroup that have left the kernel
constexpr int H_OVF2 = H_OVF + 2;          // tiles of this workgroup with more matches than small_cap
constexpr int H_WORDS = H_OVF + 8;

// Error channel: flags are OR-ed into the control header in DEVICE memory (ordinary device atomics; the last
// workgroup to leave copies them to the host-mapped result words with plain stores).
struct ErrCh {
    unsigned *word;
    unsigned spin_max;
};
__device__ __forceinline__ void err_set(const ErrCh &e, unsigned code) {
    __hip_atomic_fetch_or(e.word, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned lds_load(const unsigned *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store(unsigned *p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// Spin (bounded) until *p == want.  Wave-uniform: every lane reads the same word.
__device__ __forceinline__ bool lds_wait_eq(const unsigned *p, unsigned want, const ErrCh &err, unsigned code) {
    unsigned spins = 0;
    while (lds_load(p) != want) {
        if (++spins >= err.spin_max) { err_set(err, code); return false; }
        __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return true;
}

// ---------------------------------------------------------------------------
// Record placement.  The record array is a HEAP, the tile index is what is ordered: tile t's records are the
// tile_index[t] >> 40 words (records) that start at tile_index[t] & (2^40 - 1), in (position, pattern length) order;
// tiles are placed wherever their workgroup's current chunk of the array has room.  A workgroup owns a CHUNK of the
// array at a time, taken from one global cursor with a single atomic (and one spare chunk is always on order, so
// the atomic's round trip is never waited for); tiles fill the chunk back to back, a batch that does not fit in the
// rest of the chunk continues in the next one from the first tile that does not fit, a batch larger than a chunk
// gets an exact allocation of its own.
//
// Why not one globally contiguous, sorted array: that needs every batch's first record index = the matches of ALL
// earlier batches, i.e. a prefix over batches that are being scanned by other workgroups at the same time.  Both
// forms of it were built and measured (decoupled look-back over 64-batch windows; per-generation totals with one
// hop per 256 batches): with two rounds of staging as slack, every workgroup still ends up waiting for the slowest
// one of its generation, round after round -- 12 % of the match-dense headline and 15-25 % of the sparse workloads
// (ablation build PFAC_ABL_NOLB vs the full kernel).  Consumers lose nothing: they walk the tile index in order
// (pfac_records_expand / pfac_records_d2h deliver one sorted pfac_record array, pfac_emit_packed prints from the
// heap directly), the gaps are below 1 % of the array, and the chunk atomics are a few per microsecond.
constexpr unsigned long long TIX_BASE_MASK = (1ull << 40) - 1;   // tile index word = first record | count << 40
constexpr int TIX_CNT_SHIFT = 40;

// ---------------------------------------------------------------------------
// One step of the perfect-hash lookup (master_kernel.cu:52-63): returns the
// next state or -1.  HT/val are interleaved as int2 {owner row, next state}.
// W8: PHF width 256 (the benchmark width) -> row == state, col == byte.
template <bool W8>
__device__ __forceinline__ int phf_step(const int *R, const int2 *T, int state, int ch, int wbit, int ht_size) {
    int row, idx;
    if (W8) {
        row = state;
        idx = R[state] + ch;
    } else {
        const int key = (state << 8) | ch;
        row = key >> wbit;
        idx = R[row] + (key & ((1 << wbit) - 1));
    }
    if ((unsigned)idx >= (unsigned)ht_size) return -1;
    const int2 e = T[idx];
    return e.x == row ? e.y : -1;
}

// NWALK independent walks per lane, stepped together.  Walk w starts at tile-local position pos[w];
// n[w] counts the final states reached; m[w][..] keeps the latest MREG of them as a shift register, m[w][0] the latest
// (= all of them, in reverse walk order, when n[w] <= MREG).  lim = first tile-local byte that may not be read.
//  * all lanes step in lock step (trip count = deepest walk in the wave); dead lanes are predicated with
//    selects instead of nested divergent branches -- far fewer exec-mask / scalar instructions per step;
//  * input bytes come four at a time from one aligned 8-byte LDS read, so a step's only dependent
//    accesses are R and T (or one dense-row lookup for the second byte);
//  * NWALK = 2 (tables gathered through L2): every table round trip has an independent twin in flight --
//    the memory-level parallelism of twice the occupancy without the LDS more waves would need.  With
//    the tables in LDS a second walk buys nothing (measured), so NWALK = 1 there.
//  * FUSED (tables gathered through L2, PHF width >= 256): each slot also carries r[] of the state it leads to,
//    so a step is ONE 16-byte gather instead of a 4-byte one (r) and a dependent 8-byte one (T) -- the
//    dictionary-on-text regime is bound by the L2's request rate (every lane of a gather is its own request), and
//    this halves the requests; only the first hashed step of a walk still looks r[] up.
//  * NWALK = 4 (the dense-match regime on L2 tables, e.g. a dictionary on text): a walk there is a chain of L2
//    round trips and the wave has nothing else to do, so four chains per lane run side by side; the first
//    MREG = 4 final states of a walk stay in registers (two otherwise) -- a position where more patterns start
//    costs a second, serial walk (walk_store).
//  * ROOT == 1 (one byte leads out of the root): every survivor's first state is the same one and the dense row is
//    row 0, so the root-row and row-index lookups -- two dependent LDS round trips per round -- disappear.
//  * deepf[w] == false (a SHALLOW-FINAL survivor, see the level-2 filter): the walk accounts for its depth-1 state
//    and stops there.
template <bool W8, int NWALK, bool FUSED, int MREG, int ROOT>
__device__ __forceinline__ void walkN(const unsigned char *tile, const int *s0, int root_state, const unsigned char *d1idx,
                                      const unsigned char *colmap, unsigned d1_stride, const int *D1, bool dense1, const int2 *D1R2, const int *S0R, const int *R, const int2 *T, const int4 *T4,
                                      const unsigned (&pos)[NWALK], const bool (&active)[NWALK], const bool (&deepf)[NWALK],
                                      unsigned lim, int wbit,
                                      int ht_size, int num_final, int rn_bias, bool skip_s0, unsigned (&n)[NWALK], unsigned (&m)[NWALK][MREG]) {
    static_assert(MREG == 2 || MREG == 4, "two or four final states per walk in registers");
    const unsigned *t32 = reinterpret_cast<const unsigned *>(tile);
    unsigned win[NWALK], left[NWALK], f[NWALK];                // left: bytes the walk may still read after its first
    int s[NWALK], rn[NWALK];                                   // rn: r[row of s] (FUSED)
    // (not with four walks per lane, the dense-match regime: there the tests cost more issue slots than the gathers they save
    // cost time -- the dictionary on text measured 3.5 % slower with them)
    constexpr bool USE_CM = FUSED && NWALK < 4;
    unsigned cm[NWALK];                                        // FUSED: child mask of s -- bit (b & 31) set iff s has an edge on some byte
                                                               // congruent to b mod 32 (all ones where it is not known): a walker whose next
                                                               // byte's bit is clear is dead WITHOUT the L2 round trip that would say so
    bool go[NWALK];
    unsigned k = 0;                                            // transitions made so far (the same for every walk: a scalar)
    const int sub = wbit - 8;                                  // FUSED needs wbit >= 8: row = state >> sub
    int4 e4[NWALK];                                            // the fused slots of the last gather
#pragma unroll
    for (int w = 0; w < NWALK; w++) {
        const unsigned lo = t32[pos[w] >> 2], hi = t32[(pos[w] >> 2) + 1];   // may run a few bytes past lim: never used
        win[w] = __builtin_amdgcn_alignbyte(hi, lo, pos[w] & 3u);          // bytes pos .. pos+3
    }
#pragma unroll
    for (int w = 0; w < NWALK; w++) {
        // (dense second byte and no 1-byte pattern: the depth-1 state itself is never looked at -- any live, non-final value will do)
        const int st = ROOT == 1 ? root_state : (skip_s0 ? num_final : s0[win[w] & 0xFFu]);
        f[w] = ROOT == 1 ? 0u : d1idx[win[w] & 0xFFu];        // dense row of that state (when dense1)
        s[w] = active[w] ? st : -1;
        n[w] = 0;
#pragma unroll
        for (int k = 0; k < MREG; k++) m[w][k] = 0;
        left[w] = (deepf[w] && lim > pos[w] + 1u) ? lim - pos[w] - 1u : 0u;
        go[w] = false;
        rn[w] = 0;
        cm[w] = 0xFFFFFFFFu;
    }
    // account for the states just reached; false when no lane of the wave can go on.
    // final <=> (unsigned)s < num_final, which also rejects the dead state -1.
    // masked (FUSED): byte `bi` of the window is the NEXT byte of the walk; a walker whose state has no edge on any byte
    // congruent to it mod 32 (child mask) is dead here and now -- no gather, and the loop can end a step earlier
    auto reached = [&](int bi, bool masked) -> bool {
        bool any = false;
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            const bool fin = (unsigned)s[w] < (unsigned)num_final;
            // the latest MREG final states as a shift register (m[0] = latest): one select each, no index compare;
            // the caller puts them back in walk order
#pragma unroll
            for (int j = MREG - 1; j > 0; j--) m[w][j] = fin ? m[w][j - 1] : m[w][j];
            m[w][0] = fin ? (unsigned)s[w] : m[w][0];
            n[w] += fin ? 1u : 0u;
            go[w] = s[w] >= 0 && k < left[w];
            if (USE_CM && masked) go[w] = go[w] && ((cm[w] >> ((win[w] >> (8 * bi)) & 31u)) & 1u) != 0u;
            any = any || go[w];
        }
        return __any(any);
    };
    // fused slot number i (biased: >= 0, see ScanArgs::rn_bias) by a 32-bit byte offset from the scalar base -- one
    // shift, no 64-bit address arithmetic per lane
    auto slot = [&](int i) -> int4 {
        return *reinterpret_cast<const int4 *>(reinterpret_cast<const unsigned char *>(T4) + ((unsigned)i << 4));
    };
    // one transition on byte number `bi` of the window (straight-line: dead lanes look up a harmless, valid slot)
    auto step = [&](int bi) {
        int row[NWALK], idx[NWALK];
        if (FUSED) {
            constexpr bool MASKED = NWALK == 4 || MASK_GATHERS;
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                const int ch = (int)((win[w] >> (8 * bi)) & 0xFFu);
                // (masked gathers: a dead lane loads nothing, so its index need not be a valid one)
                const int sg = MASKED ? s[w] : (go[w] ? s[w] : 0);
                const int rg = MASKED ? rn[w] : (go[w] ? rn[w] : 0);
                if (W8) {
                    row[w] = sg;
                    idx[w] = rg + ch;
                } else {
                    row[w] = sg >> sub;
                    idx[w] = rg + (((sg & ((1 << sub) - 1)) << 8) | ch);
                }
            }
            // (a live walker's index is inside the slot array: it is padded to max(r) + width entries, and
            // pfac_repack_kernel checked every displacement and state of the image)
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                // (set before every gather although a dead lane's slot is only ever selected under go[w]: measured 15 %
                // faster than carrying the stale value -- the gather then has no dependence on the register's old content)
                e4[w] = make_int4(-1, -1, 0, 0);
                if (MASKED) {
                    // dead lanes stay out of the gather: every lane of a gather costs the texture path an address
                    // cycle (64 per wave-instruction, against 16 for a coalesced 1 KiB load), and a round's later
                    // steps have few walkers left
                    if (go[w]) e4[w] = slot(idx[w]);
                } else {
                    e4[w] = slot(idx[w]);
                }
            }
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                s[w] = (go[w] && e4[w].x == row[w]) ? e4[w].y : -1;
                rn[w] = e4[w].z;
                cm[w] = (unsigned)e4[w].w;
            }
            k++;
            return;
        }
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            const int ch = (int)((win[w] >> (8 * bi)) & 0xFFu);
            const int sg = go[w] ? s[w] : 0;
            if (W8) {
                row[w] = sg;
                idx[w] = R[sg] + ch;
            } else {
                const int key = (sg << 8) | ch;
                row[w] = key >> wbit;
                idx[w] = R[row[w]] + (key & ((1 << wbit) - 1));
            }
        }
        int2 e[NWALK];
        unsigned ic[NWALK];
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            ic[w] = min((unsigned)idx[w], (unsigned)ht_size - 1u);     // (the table ends at its last used slot)
            e[w] = T[ic[w]];
        }
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            s[w] = (go[w] && ic[w] == (unsigned)idx[w] && e[w].x == row[w]) ? e[w].y : -1;
        }
        k++;
    };
    // FUSED: the first hashed step of a walk has no slot to take r[] from
    auto load_rn = [&]() {
        if (FUSED) {
#pragma unroll
            for (int w = 0; w < NWALK; w++) rn[w] = R[(go[w] ? s[w] : 0) >> sub] + rn_bias;
        }
    };
    if (!reached(1, false)) return;
    if (dense1) {
        // second byte: the depth-1 state's row is dense in LDS -- one lookup, no hash, no owner check.  Stage by stage for
        // all the walks of the lane (column, row entry, packed r[] / child mask): written walk by walk, the uniform test on
        // D1R2 put every walk into basic blocks of its own and their LDS round trips in SERIES -- six trips instead of three
        unsigned col[NWALK];
        int nx[NWALK];
#pragma unroll
        for (int w = 0; w < NWALK; w++) col[w] = colmap[(win[w] >> 8) & 0xFFu];
#pragma unroll
        for (int w = 0; w < NWALK; w++) nx[w] = D1[(go[w] ? f[w] : 0u) * d1_stride + col[w]];
        if (FUSED && D1R2) {
            // packed entry: the depth-2 state and where its r[] sits in LDS -- the walk's first hashed step needs no r[]
            // gather either
            bool ok[NWALK];
            int2 e2[NWALK];
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                ok[w] = go[w] && nx[w] >= 0;
                e2[w] = D1R2[ok[w] ? (nx[w] >> D1_STATE_BITS) : 0];        // {r[] of the depth-2 state, its child mask}
            }
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                s[w] = ok[w] ? (nx[w] & ((1 << D1_STATE_BITS) - 1)) : -1;
                rn[w] = e2[w].x;
                cm[w] = (unsigned)e2[w].y;
            }
        } else {
#pragma unroll
            for (int w = 0; w < NWALK; w++) s[w] = go[w] ? nx[w] : -1;
        }
        k++;
    } else {
        if (FUSED && S0R) {
            // too many depth-1 states for dense rows: their r[] at least sits in LDS (by root byte), so the second
            // byte costs one gather, not two
#pragma unroll
            for (int w = 0; w < NWALK; w++) rn[w] = S0R[win[w] & 0xFFu];
        } else {
            load_rn();
        }
        step(1);
    }
    if (!reached(2, true)) return;
    if (dense1 && !(FUSED && D1R2)) load_rn();
    step(2);
    if (!reached(3, true)) return;
    step(3);
    for (;;) {                                                 // deeper than 4 bytes: next aligned windows
        if (!reached(0, false)) return;
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            const unsigned p = pos[w] + 1u + k;                // next byte of the walk
            const unsigned lo = t32[p >> 2], hi = t32[(p >> 2) + 1];
            win[w] = __builtin_amdgcn_alignbyte(hi, lo, p & 3u);
        }
        if (USE_CM) {                                          // the child masks against the first byte of the new windows
            bool any = false;
#pragma unroll
            for (int w = 0; w < NWALK; w++) {
                go[w] = go[w] && ((cm[w] >> (win[w] & 31u)) & 1u) != 0u;
                any = any || go[w];
            }
            if (!__any(any)) return;
        }
        step(0);
        if (!reached(1, true)) return;
        step(1);
        if (!reached(2, true)) return;
        step(2);
        if (!reached(3, true)) return;
        step(3);
    }
}

// One record into the global array (the DIRECT paths), in the scan's record form.
__device__ __forceinline__ void put_record(const ScanArgs &a, unsigned long long ri, unsigned tpos, unsigned gpos, unsigned state) {
    if (ri >= a.out_cap) return;
    if (a.rec_bytes == 2) {
        static_cast<unsigned short *>(a.out)[ri] = (unsigned short)(tpos | (state << 12));
    } else if (a.rec_bytes == 4) {
        static_cast<unsigned *>(a.out)[ri] = tpos | (state << 12);
    } else {
        pfac_record rec;
        rec.pos = gpos;
        rec.state = state;
        static_cast<pfac_record *>(a.out)[ri] = rec;
    }
}

// One record into a tile's LDS staging buffer, in the packed format.  S16 (the kernels with their tables in LDS, where
// the small automata with 16-bit records run): 16-bit records are staged as 16-bit words, so that copy_out moves them
// to global memory as they lie.  Else, and for the wider packed form, as 32-bit words (the L2-table kernels are paced
// by their instruction stream and registers: they keep the one form).
template <bool S16>
__device__ __forceinline__ void stage_put(const ScanArgs &a, unsigned *stage, unsigned i, unsigned v) {
    if (S16 && a.rec_bytes == 2) reinterpret_cast<unsigned short *>(stage)[i] = (unsigned short)v;
    else stage[i] = v;
}

// Same walk for the rare offsets where more patterns start than the fast walk keeps final states in registers:
// every final state goes to the LDS staging buffer (packed) or straight to global memory.
template <bool W8, bool DIRECT, bool S16>
__device__ __forceinline__ void walk_store(const ScanArgs &a, const unsigned char *tile, const int *s0, const int *R, const int2 *T,
                                           unsigned pos, unsigned lim, unsigned *stage, unsigned long long ri, unsigned gpos) {
    unsigned n = 0;
    int s = s0[tile[pos]];
    unsigned p = pos + 1;
    while (s >= 0) {
        if (s < a.num_final) {
            if (DIRECT) put_record(a, ri + n, pos, gpos, (unsigned)s);
            else if (ri + n < a.stage_cap) stage_put<S16>(a, stage, (unsigned)ri + n, pos | ((unsigned)s << 12));
            n++;
        }
        if (p >= lim) break;
        s = phf_step<W8>(R, T, s, tile[p], a.wbit, a.ht_size);
        p++;
    }
}

struct Dense1 {
    const unsigned char *colmap;
    const unsigned char *idx;
    const int *rows;
    bool on;
    const int2 *r2;     // packed rows (FUSED): {r[], child mask} of the depth-2 states, in LDS; null = plain rows
    const int *s0r;     // no dense rows (FUSED): r[] of the depth-1 state each root byte leads to, in LDS; else null
};

// One round: up to 64*NWALK FIFO entries [q0, q0+nact), lane L takes entries L, L+64, ... side by side; their records
// are appended, in queue (= position) order, at index `wrun` of the staging buffer (DIRECT == false) or of the global
// record array.  Entries without QDEEP are shallow-final survivors: one record, the depth-1 state of their byte; a
// round made of those alone needs neither a walk nor a prefix sum.  Returns the number of records.
template <bool W8, bool DIRECT, int NWALK, bool FUSED, int ROOT, bool S16>
__device__ __forceinline__ unsigned roundN(const ScanArgs &a, const unsigned char *tile, const int *s0, const Dense1 &d1,
                                           const int *R, const int2 *T, const unsigned short *q, unsigned q0,
                                           unsigned nact, int lane, unsigned *stage, unsigned lim,
                                           unsigned long long tile_base, unsigned long long wrun) {
    static_assert(NWALK >= 1 && NWALK <= 4, "one to four walks per lane");
    constexpr int MREG = NWALK == 4 ? 4 : 2;
    bool active[NWALK], deepf[NWALK];
    unsigned pos[NWALK], n[NWALK], m[NWALK][MREG];
    bool anydeep = false;
#pragma unroll
    for (int w = 0; w < NWALK; w++) {
        active[w] = (unsigned)lane + WAVE * w < nact;
        const unsigned e = active[w] ? q[q0 + WAVE * w + lane] : 0u;
        pos[w] = e & 0xFFFu;
        deepf[w] = (e & QDEEP) != 0;
        anydeep = anydeep || deepf[w];
    }
#ifdef PFAC_ABL_NOWALK                         // ablation builds only: deep entries are treated as shallow (wrong records)
    anydeep = false;
#endif
    if (!__any(anydeep)) {
#pragma unroll
        for (int w = 0; w < NWALK; w++) {
            if (!active[w]) continue;
            const unsigned st = ROOT == 1 ? (unsigned)a.root_state : (unsigned)s0[tile[pos[w]]];
            const unsigned long long ri = wrun + WAVE * w + lane;
            if (DIRECT) put_record(a, ri, pos[w], (unsigned)tile_base + pos[w], st);
            else if (ri < a.stage_cap) stage_put<S16>(a, stage, (unsigned)ri, pos[w] | (st << 12));
        }
        return nact;
    }
    walkN<W8, NWALK, FUSED, MREG, ROOT>(tile, s0, a.root_state, d1.idx, d1.colmap, (unsigned)a.d1_stride, d1.rows, d1.on, d1.r2, d1.s0r, R, T, a.T4, pos, active, deepf, lim,
                                        a.wbit, a.ht_size, a.num_final, a.rn_bias, ROOT != 1 && d1.on && a.sec_filter != 0, n, m);
    // the walk kept its latest MREG final states as a shift register (m[0] = latest): back into walk order
#pragma unroll
    for (int w = 0; w < NWALK; w++) {
        const unsigned c = n[w];
        if (MREG == 4) {
            const unsigned a0 = m[w][0], a1 = m[w][1], a2 = m[w][2], a3 = m[w][3];
            m[w][0] = c >= 4u ? a3 : (c == 3u ? a2 : (c == 2u ? a1 : a0));
            m[w][1] = c >= 4u ? a2 : (c == 3u ? a1 : a0);
            m[w][2] = c >= 4u ? a1 : a0;
            m[w][3] = a0;
        } else {
            const unsigned a0 = m[w][0], a1 = m[w][1];
            m[w][0] = c >= 2u ? a1 : a0;
            m[w][1] = a0;
        }
    }
    // prefix sums of the counts, two walks per scan (16-bit fields; a walk reports < 1024 matches)
    unsigned ex[NWALK], total = 0;
#pragma unroll
    for (int w0 = 0; w0 < NWALK; w0 += 2) {
        const bool pair = w0 + 1 < NWALK;
        const unsigned packed = pair ? (n[w0] | (n[pair ? w0 + 1 : w0] << 16)) : n[w0];
        const unsigned inc = wave_incl_scan(packed);
        const unsigned last = bcast_last(inc);
        const unsigned t0 = pair ? (last & 0xFFFFu) : last;
        ex[w0] = total + (pair ? (inc & 0xFFFFu) : inc) - n[w0];
        total += t0;
        if (pair) {
            ex[w0 + 1] = total + (inc >> 16) - n[w0 + 1];
            total += last >> 16;
        }
    }
#pragma unroll
    for (int w = 0; w < NWALK; w++) {
        const bool regs = n[w] <= (unsigned)MREG;              // every record of this walk is in registers
        const unsigned gpos = (unsigned)tile_base + pos[w];
        if (DIRECT) {
            const unsigned long long ri = wrun + ex[w];
            if (regs && n[w] > 0) put_record(a, ri, pos[w], gpos, m[w][0]);
#pragma unroll
            for (int k = 1; k < MREG; k++)
                if (regs && n[w] > (unsigned)k) put_record(a, ri + k, pos[w], gpos, m[w][k]);
            if (!regs) walk_store<W8, true, S16>(a, tile, s0, R, T, pos[w], lim, nullptr, ri, gpos);
        } else {
            const unsigned ri = (unsigned)wrun + ex[w];        // tile-local record index: 32 bits are plenty
            if (regs && n[w] > 0 && ri < a.stage_cap) stage_put<S16>(a, stage, ri, pos[w] | (m[w][0] << 12));
#pragma unroll
            for (int k = 1; k < MREG; k++)
                if (regs && n[w] > (unsigned)k && ri + k < a.stage_cap) stage_put<S16>(a, stage, ri + k, pos[w] | (m[w][k] << 12));
            if (!regs) walk_store<W8, false, S16>(a, tile, s0, R, T, pos[w], lim, stage, ri, 0);
        }
    }
    return total;
}

// Compaction + walk over one wave tile.  keep[j] = the survivors of half-tile j that yield a record or need a walk
// (bit b = byte b of the lane's 32), deep[j] = those of them that need the walk.  Kept survivors are appended, in
// position order, to a FIFO in LDS; whenever 64 are pending a full round runs, so lanes stay busy even when only
// one offset in thirteen survives the root test.  Returns the tile's match count; with DIRECT the records are
// written at global index wrun onwards.
template <bool W8, bool DIRECT, int NWALK, bool FUSED, int ROOT>
__device__ __forceinline__ unsigned long long tile_pass(const ScanArgs &a, const unsigned char *tile, const int *s0,
                                                        const Dense1 &d1, const int *R, const int2 *T, unsigned short *q,
                                                        unsigned *stage, const unsigned (&keep)[MSUBS],
                                                        const unsigned (&deep)[MSUBS], int lane,
                                                        unsigned lim, unsigned long long tile_base,
                                                        unsigned long long wrun) {
    unsigned head = 0, tail = 0;               // pending survivors: q[head, tail), always fewer than one round between appends
    constexpr bool S16 = NWALK == 1;           // the kernels with their tables in LDS: 16-bit staging (stage_put)
    // per-lane survivor counts of the 2 half-tiles, prefix-summed in one packed DPP scan (16-bit fields: a
    // half-tile holds at most 2048 survivors)
    static_assert(MSUBS == 2, "the packed scan assumes 2 half-tiles");
    const unsigned c0 = __popc(keep[0]), c1 = __popc(keep[1]);
    const unsigned pa = wave_incl_scan(c0 | (c1 << 16));
    const unsigned incls[MSUBS] = {pa & 0xFFFFu, pa >> 16};
    const unsigned cnts[MSUBS] = {c0, c1};
    const unsigned la = bcast_last(pa);
    const unsigned totals[MSUBS] = {la & 0xFFFFu, la >> 16};
    if (ROOT == 1 && !__any((deep[0] | deep[1]) != 0u)) {
        // No deep survivor in the tile (the usual case for a sparse pattern set): every kept survivor is exactly one
        // record, the depth-1 state -- written straight to its slot, in position order; no FIFO, no rounds.
        const unsigned st = (unsigned)a.root_state;
#pragma unroll
        for (int j = 0; j < MSUBS; j++) {
            if (totals[j] == 0) continue;
            const unsigned lpos = j * MSUB + lane * MLANE;
            unsigned o = (j ? totals[0] : 0u) + incls[j] - cnts[j];
#ifdef PFAC_ABL_NOSTAGE                        // ablation builds only: counted, never staged (stale records)
            if (true) continue;
#endif
            if (!DIRECT && totals[0] + totals[1] <= a.stage_cap) {
                // everything fits (else the tile is walked again, DIRECT): no bound checks, two records per trip
                const unsigned w0 = lpos | (st << 12);
                if (S16 && a.rec_bytes == 2) {
                    unsigned short *s16 = reinterpret_cast<unsigned short *>(stage);
                    for (unsigned m = keep[j]; m;) {
                        s16[o] = (unsigned short)(w0 + (unsigned)__ffs(m) - 1u);
                        m &= m - 1;
                        if (m) s16[o + 1] = (unsigned short)(w0 + (unsigned)__ffs(m) - 1u);
                        m &= m - 1;
                        o += 2;
                    }
                    continue;
                }
                for (unsigned m = keep[j]; m;) {
                    stage[o] = w0 + (unsigned)__ffs(m) - 1u;
                    m &= m - 1;
                    if (m) stage[o + 1] = w0 + (unsigned)__ffs(m) - 1u;
                    m &= m - 1;                         // (0 stays 0)
                    o += 2;
                }
                continue;
            }
            for (unsigned m = keep[j]; m; m &= m - 1) {
                const unsigned pos = lpos + (__ffs(m) - 1);
                if (DIRECT) put_record(a, wrun + o, pos, (unsigned)tile_base + pos, st);
                else if (o < a.stage_cap) stage_put<S16>(a, stage, o, pos | (st << 12));
                o++;
            }
        }
        return wrun + totals[0] + totals[1];
    }
    constexpr unsigned RW = WAVE * NWALK;      // survivors per round
#ifdef PFAC_TRACE_BUILD
    unsigned long long tp_round = 0, tp_n = 0, tp_t0 = __builtin_amdgcn_s_memrealtime();
#define TP_ROUND(call) do { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); call; tp_round += __builtin_amdgcn_s_memrealtime() - t_; tp_n++; } while (0)
#else
#define TP_ROUND(call) do { call; } while (0)
#endif
#pragma unroll
    for (int j = 0; j < MSUBS; j++) {
        const unsigned mask = keep[j];
        const unsigned dmask = deep[j];
        const unsigned cnt = cnts[j];
        const unsigned incl = incls[j];
        const unsigned S = totals[j];
        if (S == 0) continue;
        const unsigned lpos = j * MSUB + lane * MLANE;
        // A half-tile with more than 512 survivors is appended in four groups of 16 lanes (16 * 32 = 512 positions,
        // in position order), so the FIFO needs one round's left-overs + 512 slots only.
        const int ngrp = S > 512u ? 4 : 1;
        for (int gi = 0; gi < ngrp; gi++) {
            unsigned gbase = 0, gcnt = S;
            bool mine = true;
            if (ngrp != 1) {
                gbase = gi ? __builtin_amdgcn_readlane(incl, 16 * gi - 1) : 0u;
                gcnt = __builtin_amdgcn_readlane(incl, 16 * gi + 15) - gbase;
                mine = (lane >> 4) == gi;
            }
            if (tail + gcnt > (unsigned)QCAP) {    // no room behind the pending entries (fewer than one round of them): move them to the front
                const unsigned rem = tail - head;
                unsigned short v[NWALK];
#pragma unroll
                for (int w = 0; w < NWALK; w++) v[w] = (unsigned)lane + WAVE * w < rem ? q[head + WAVE * w + lane] : (unsigned short)0;
                wave_lds_sync();
#pragma unroll
                for (int w = 0; w < NWALK; w++) if ((unsigned)lane + WAVE * w < rem) q[WAVE * w + lane] = v[w];
                head = 0;
                tail = rem;
            }
            if (mine) {
                unsigned o = tail + (incl - cnt) - gbase;
                for (unsigned m = mask; m; m &= m - 1) {
                    const unsigned b = __ffs(m) - 1;
                    q[o++] = (unsigned short)((lpos + b) | (((dmask >> b) & 1u) << 15));
                }
            }
            tail += gcnt;
            wave_lds_sync();
            for (; head + RW <= tail; head += RW)
                TP_ROUND((wrun += roundN<W8, DIRECT, NWALK, FUSED, ROOT, S16>(a, tile, s0, d1, R, T, q, head, RW, lane, stage, lim, tile_base, wrun)));
        }
    }
    // (the last, partial round runs where its entries lie: nothing is appended behind them any more; with two walks per
    // lane and at most 64 entries left, the one-walk form of the round does the same work in half the instructions -- the
    // sparse L2-table kernels are paced by their instruction stream, and their typical tile ends on such a round)
    if (tail > head) {
        if (NWALK == 2 && !DIRECT && tail - head <= (unsigned)WAVE)
            TP_ROUND((wrun += roundN<W8, DIRECT, 1, FUSED, ROOT, S16>(a, tile, s0, d1, R, T, q, head, tail - head, lane, stage, lim, tile_base, wrun)));
        else
            TP_ROUND((wrun += roundN<W8, DIRECT, NWALK, FUSED, ROOT, S16>(a, tile, s0, d1, R, T, q, head, tail - head, lane, stage, lim, tile_base, wrun)));
    }
#ifdef PFAC_TRACE_BUILD
    if (!DIRECT && a.dbg && blockIdx.x < 8 && lane == 0 && (threadIdx.x >> 6) == 0) {
        // compute wave 0 of the first 8 workgroups: accumulated over the launch (slot 31 of the block's first row)
        unsigned long long *acc = a.dbg + (size_t)blockIdx.x * 64 * 32 + 10;      // columns 10..14 of the block's row 0
        acc[0] += tp_round; acc[1] += tp_n; acc[2] += __builtin_amdgcn_s_memrealtime() - tp_t0; acc[3] += 1; acc[4] += tail - head;
    }
#endif
    return wrun;
}

// Staged words of one tile -> global memory, in order (packed format only: the staged word IS the record).  Four
// records (16 bytes) per lane per store, aligned to the record array; non-temporal stores -- the records are not read
// again by this launch, and written through they do not pile up dirty in L2 until the kernel ends (measured: the same at
// 1 GiB shards, +3.5 % at 4 GiB).
template <bool SPARSE>
__device__ __forceinline__ void copy_out(const ScanArgs &a, const unsigned *stage, unsigned cnt, unsigned long long base, int lane) {
    if (cnt == 0) return;
#ifdef PFAC_ABL_NOEMIT                         // ablation builds only: records never leave LDS
    return;
#endif
    if (a.rec_bytes == 2 && !SPARSE) {
        // automata with at most 16 final states, tables in LDS: 16-bit staged words, and every run starts on a 16-byte
        // boundary of the record array (the heap hands out multiples of 8 records), so it leaves as whole 16-byte
        // blocks, one ds_read_b128 and one store per lane; the last block carries whatever the staging buffer holds past
        // cnt into the run's own padding (stage_cap is a multiple of 8)
        const unsigned short *s16 = reinterpret_cast<const unsigned short *>(stage);
        unsigned short *out = static_cast<unsigned short *>(a.out);
        if (((unsigned)base & 7u) != 0u || base + ((cnt + 7u) & ~7u) > a.out_cap) {
            for (unsigned i = (unsigned)lane; i < cnt; i += WAVE)       // the record array ends inside this run: checked
                if (base + i < a.out_cap) out[base + i] = s16[i];
            return;
        }
        for (unsigned i = 8u * (unsigned)lane; i < cnt; i += 8u * WAVE)
            __builtin_nontemporal_store(*reinterpret_cast<const u32x4 *>(s16 + i), reinterpret_cast<u32x4 *>(out + base + i));
        return;
    }
    if (a.rec_bytes == 2) {
        // the same records staged as 32-bit words (the L2-table kernels): the record is the low half of the staged word;
        // eight per 16-byte store, the ragged head and tail one lane each (none when the run is aligned)
        unsigned short *out = static_cast<unsigned short *>(a.out);
        if (base + cnt > a.out_cap) {
            for (unsigned i = (unsigned)lane; i < cnt; i += WAVE)
                if (base + i < a.out_cap) out[base + i] = (unsigned short)stage[i];
            return;
        }
        unsigned head = (0u - (unsigned)base) & 7u;
        head = head < cnt ? head : cnt;
        if ((unsigned)lane < head) out[base + lane] = (unsigned short)stage[lane];
        unsigned i = head + 8u * (unsigned)lane;
        for (; i + 8u <= cnt; i += 8u * WAVE) {
            const u32x4 v = {(stage[i] & 0xFFFFu) | (stage[i + 1] << 16), (stage[i + 2] & 0xFFFFu) | (stage[i + 3] << 16),
                             (stage[i + 4] & 0xFFFFu) | (stage[i + 5] << 16), (stage[i + 6] & 0xFFFFu) | (stage[i + 7] << 16)};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(out + base + i));
        }
        const unsigned tail = head + ((cnt - head) & ~7u);
        if (tail + (unsigned)lane < cnt) out[base + tail + lane] = (unsigned short)stage[tail + lane];
        return;
    }
    if (SPARSE && cnt <= 2u * WAVE && base + cnt <= a.out_cap) {
        // a sparse tile (the L2-table workloads: tens of records): one record per lane per store, two independent trips
        // -- the aligned 16-byte form below pays three dependent LDS round trips (head, body, tail) for a few hundred bytes
        unsigned *out = static_cast<unsigned *>(a.out);
        const unsigned v0 = (unsigned)lane < cnt ? stage[lane] : 0u, v1 = (unsigned)lane + WAVE < cnt ? stage[lane + WAVE] : 0u;
        if ((unsigned)lane < cnt) __builtin_nontemporal_store(v0, out + base + lane);
        if ((unsigned)lane + WAVE < cnt) __builtin_nontemporal_store(v1, out + base + lane + WAVE);
        return;
    }
    unsigned *out = static_cast<unsigned *>(a.out);
    if (base + cnt > a.out_cap) {              // the record array ends inside this tile: word by word, checked
        for (unsigned i = (unsigned)lane; i < cnt; i += WAVE)
            if (base + i < a.out_cap) out[base + i] = stage[i];
        return;
    }
    unsigned head = (0u - (unsigned)base) & 3u;                // records up to the next 16-byte boundary of the array
    head = head < cnt ? head : cnt;
    if ((unsigned)lane < head) out[base + lane] = stage[lane];
    unsigned i = head + 4u * (unsigned)lane;
    for (; i + 4u <= cnt; i += 4u * WAVE) {
        const u32x4 v = {stage[i], stage[i + 1], stage[i + 2], stage[i + 3]};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(out + base + i));
    }
    const unsigned tail = head + ((cnt - head) & ~3u);         // the last 1..3 records: one lane each
    if (tail + (unsigned)lane < cnt) out[base + tail + lane] = stage[tail + lane];
}

// ---------------------------------------------------------------------------
// Dense mode, second form (a dictionary on text: most offsets start a walk, every third goes beyond its second byte).
// tile_pass runs its walkers in rounds of 256, in lock step to the depth of the round's deepest walker -- on text a
// fifth of the lane-steps of such a round belong to a live walker -- because a round's records have to come out in
// (position, length) order, and its 8 KiB staging buffer per wave leaves room for 9 waves per CU.  Here the order is
// made afterwards, and the records wait in device memory, not in LDS (15 waves per CU):
//   * front end, D2_FB x 64 consecutive positions per trip, every lane busy: root table (final state of the first byte |
//     word offset of its dense row), column of the second byte -> dense row entry -> packed {r[], child mask}: three
//     dependent LDS trips; the final states of depth 1 and 2 are logged at once; the positions whose depth-2 state has an
//     edge on a byte congruent to the third one (child mask) go into a ring of pending walkers {position, state, fused
//     slot of the first gather, records so far};
//   * PFAC_D2_NS walker slots per lane; a slot whose walk has ended takes the next ring entry, so the gathers of a step
//     belong to live walkers only; a walker dies WITHOUT the gather that would say so when the child mask of its state
//     has no bit for the next byte; every final state is logged as {position, k-th record of the position, state};
//   * the log is the wave's own scratch in device memory, written 64 words at a time from an LDS staging area (a store of
//     a handful of lanes costs the texture path as much as a full one);
//   * once the tile is done the log is read back (into registers, where it fits): the records of every position are
//     counted (4-bit fields in LDS), the counts prefix-summed (per 8 positions + a nibble sum inside the word), and every
//     log entry is stored straight to its place in the heap: base + prefix[position] + k.
// Log full or more than 15 patterns starting at one offset: the tile is done again by tile_pass (returns ~0u), counted
// and then written directly (no staging buffer in this layout).  Needs: fused tables, packed dense rows (every depth-1
// state has a dense row, every depth-2 state an entry in d1.r2), final states below 2^16, 4-byte records.
#ifndef PFAC_D2_FB
#define PFAC_D2_FB 2
#endif
#ifndef PFAC_D2_NS
#define PFAC_D2_NS 2
#endif
constexpr int D2_FB = PFAC_D2_FB;              // front-end batches per trip (their LDS round trips overlap)
static_assert(D2_RING >= (D2_FB + 1) * WAVE, "ring: one trip's pushes on top of a batch of left-overs");
template <bool W8>
__device__ __forceinline__ unsigned dense2_tile(const ScanArgs &a, const unsigned char *tile, const unsigned *t0, const Dense1 &d1,
                                                unsigned char *aux, unsigned *logg, int lane, unsigned lim, unsigned own_end) {
    constexpr int NS = PFAC_D2_NS;             // walker slots per lane
    uint2 *ring = reinterpret_cast<uint2 *>(aux);
    const unsigned *t32 = reinterpret_cast<const unsigned *>(tile);
    const int sub = a.wbit - 8;
    const unsigned nfin = (unsigned)a.num_final, logcap = a.d2log_cap;
    // the log through a buffer descriptor: a scalar base, one shift per store, and a store past the end is dropped
    const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(logg, 0, (int)(logcap * 4u), 0x00020000);
    unsigned pos[NS], pn[NS], jn[NS];          // position; index of the byte the next gather consumes; records of the position so far
    int s[NS], idx[NS];                        // state; fused slot the next gather reads (r[row of state] + column of that byte)
    bool alive[NS];
#pragma unroll
    for (int w = 0; w < NS; w++) { pos[w] = pn[w] = jn[w] = 0u; s[w] = -1; idx[w] = 0; alive[w] = false; }
    unsigned P0 = 0, head = 0, fcount = 0, lc = 0;             // wave-uniform: next front-end position, ring, log fill
    unsigned jmax = 0;
    const unsigned no_root = 0xFFFFu | ((unsigned)(a.d1_rows * a.d1_stride) << 16);
    auto lane_rank = [&](unsigned long long b) -> unsigned {
        return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    };
    // Log words are collected in LDS (the bytes of the position counts, which only the scatter phase uses) and leave 64 at a
    // time: a store of a handful of lanes costs the texture path as much as a full one, and a tile logs ~180 handfuls
    unsigned *stg = reinterpret_cast<unsigned *>(aux + D2_CNT_OFF);
    constexpr unsigned STG = (unsigned)(WTILE / 2 / 4);        // words (a power of two)
    static_assert(STG >= (unsigned)(WAVE + 2 * D2_FB * WAVE) && STG >= (unsigned)(WAVE + PFAC_D2_NS * WAVE), "log staging: < 64 words pending + what a trip / a step adds");
    unsigned fl = 0;                                           // log words flushed so far (a multiple of 64 until the end)
    auto log_put = [&](bool f, unsigned word) {
        const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
        if (b) {
            if (f) stg[(lc + lane_rank(b)) & (STG - 1u)] = word;
            lc += (unsigned)__popcll(b);
        }
    };
    auto log_flush = [&](bool all) {
        if (lc - fl >= (unsigned)WAVE || (all && lc != fl)) {
            wave_lds_sync();
            while (lc - fl >= (unsigned)WAVE) {
                __builtin_amdgcn_raw_buffer_store_b32(stg[(fl + (unsigned)lane) & (STG - 1u)], lrs, (int)((fl + (unsigned)lane) << 2), 0, 0);
                fl += WAVE;
            }
            if (all && fl + (unsigned)lane < lc)
                __builtin_amdgcn_raw_buffer_store_b32(stg[(fl + (unsigned)lane) & (STG - 1u)], lrs, (int)((fl + (unsigned)lane) << 2), 0, 0);
        }
    };
    auto slot = [&](int i) -> int4 {
        return *reinterpret_cast<const int4 *>(reinterpret_cast<const unsigned char *>(a.T4) + ((unsigned)i << 4));
    };
    auto slot_of = [&](int rnv, unsigned st, unsigned byte) -> int {       // fused slot of (state, byte), r[row of state] given
        return W8 ? rnv + (int)byte : rnv + (int)(((st & ((1u << sub) - 1u)) << 8) | byte);
    };
    // One trip of the front end: D2_FB x 64 positions from P0 on.  EDGE: the input's last tile (positions past n_owned start
    // nothing, bytes past the input are not read) -- everywhere else a position's first three bytes are inside the tile + halo
    // and those tests fall away.  A byte that starts no pattern has the no-edge row, a (first, second) byte pair that is no
    // prefix the no-child entry of d1.r2: "no second state" needs no test of its own.
    const bool edge = own_end < (unsigned)WTILE || lim < (unsigned)WTILE + 3u;
    const unsigned n2 = (unsigned)a.d1_n2;
    auto front = [&](auto edge_c) {
        constexpr bool EDGE = decltype(edge_c)::value;
        unsigned p[D2_FB], win[D2_FB], rt[D2_FB], col[D2_FB];
        int nx[D2_FB];
        int2 e2[D2_FB];
#pragma unroll
        for (int u = 0; u < D2_FB; u++) {
            p[u] = P0 + (unsigned)(u * WAVE + lane);
            const unsigned lo = t32[p[u] >> 2], hi = t32[(p[u] >> 2) + 1];
            win[u] = __builtin_amdgcn_alignbyte(hi, lo, p[u] & 3u);              // bytes p .. p+3
        }
#pragma unroll
        for (int u = 0; u < D2_FB; u++) {
            rt[u] = t0[win[u] & 0xFFu];
            col[u] = d1.colmap[(win[u] >> 8) & 0xFFu];
        }
#pragma unroll
        for (int u = 0; u < D2_FB; u++) {
            if (EDGE && p[u] >= own_end) rt[u] = no_root;
            nx[u] = d1.rows[(rt[u] >> 16) + col[u]];                             // depth-2 state | index of its r2 entry << 20, or -1
        }
#pragma unroll
        for (int u = 0; u < D2_FB; u++) {
            if (EDGE && p[u] + 1u >= lim) nx[u] = -1;
            const unsigned ri = (unsigned)(nx[u] >> D1_STATE_BITS);             // (-1: beyond every index)
            e2[u] = d1.r2[ri < n2 ? ri : n2];                                    // {r[] of the depth-2 state, its child mask}; entry n2: {0, 0}
        }
#pragma unroll
        for (int u = 0; u < D2_FB; u++) {
            const unsigned s1 = rt[u] & 0xFFFFu, s2 = (unsigned)nx[u] & ((1u << D1_STATE_BITS) - 1u);
            const bool fin1 = s1 != 0xFFFFu, fin2 = s2 < nfin;                   // (no second state: s2 = 2^20 - 1, above every final state)
            const unsigned b2 = (win[u] >> 16) & 0xFFu;
#ifdef PFAC_ABL_D2NOWALK                       // ablation builds only: nothing goes beyond its second byte (records missing)
            const bool more = false && b2;
#else
            const bool more = (((unsigned)e2[u].y >> (b2 & 31u)) & 1u) != 0u && (!EDGE || p[u] + 2u < lim);
#endif
            log_put(fin1, p[u] | (s1 << 16));
            log_put(fin2, p[u] | (fin1 ? 1u << 12 : 0u) | ((unsigned)nx[u] << 16));
            const unsigned long long mb = __builtin_amdgcn_ballot_w64(more);
            if (mb) {
                const unsigned n12 = (fin1 ? 1u : 0u) + (fin2 ? 1u : 0u);
                if (more) ring[(head + fcount + lane_rank(mb)) & (unsigned)(D2_RING - 1)] =
                    make_uint2(p[u] | ((unsigned)nx[u] << 12), (unsigned)slot_of(e2[u].x, s2, b2) | (n12 << 28));
                fcount += (unsigned)__popcll(mb);
            }
        }
        P0 += D2_FB * WAVE;
    };
#ifdef PFAC_TRACE_BUILD                        // diagnostic build only: where a tile's time goes (compute wave 0 of the first 8 workgroups)
    unsigned long long tq_front = 0, tq_iter = 0, tq_n = 0;
    const unsigned long long tq_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    for (;;) {
        unsigned long long dm[NS];
        unsigned nd = 0;
#pragma unroll
        for (int w = 0; w < NS; w++) { dm[w] = __builtin_amdgcn_ballot_w64(!alive[w]); nd += (unsigned)__popcll(dm[w]); }
#ifdef PFAC_TRACE_BUILD
        const unsigned long long tq_a = __builtin_amdgcn_s_memrealtime();
#endif
        // ---- front end: as many trips as the free slots ask for
        while (fcount < nd && P0 < own_end && fcount <= (unsigned)(D2_RING - D2_FB * WAVE)) {
            if (edge) front(std::true_type{}); else front(std::false_type{});
            log_flush(false);
        }
#ifdef PFAC_TRACE_BUILD
        tq_front += __builtin_amdgcn_s_memrealtime() - tq_a;
        tq_n++;
#endif
        if (nd == (unsigned)(NS * WAVE) && fcount == 0u) break;        // no walker left, none pending, every position seen
        wave_lds_sync();
        // ---- free slots take the pending walkers
#pragma unroll
        for (int w = 0; w < NS; w++) {
            if (fcount && dm[w]) {
                const unsigned free_n = (unsigned)__popcll(dm[w]);
                const unsigned take = free_n < fcount ? free_n : fcount;
                const unsigned rk = lane_rank(dm[w]);
                if (!alive[w] && rk < take) {
                    const uint2 e = ring[(head + rk) & (unsigned)(D2_RING - 1)];
                    pos[w] = e.x & 0xFFFu;
                    s[w] = (int)(e.x >> 12);
                    idx[w] = (int)(e.y & 0x0FFFFFFFu);
                    jn[w] = e.y >> 28;
                    pn[w] = pos[w] + 2u;
                    alive[w] = true;
                }
                head += take;
                fcount -= take;
            }
        }
        // ---- one transition of every live walker
        int4 e4[NS];
        unsigned nb[NS];
#pragma unroll
        for (int w = 0; w < NS; w++) {
            e4[w] = make_int4(-1, -1, 0, 0);
            if (alive[w]) e4[w] = slot(idx[w]);
        }
#pragma unroll
        for (int w = 0; w < NS; w++) nb[w] = tile[alive[w] ? pn[w] + 1u : 0u];     // the byte after (at most one past lim: not used then)
#pragma unroll
        for (int w = 0; w < NS; w++) {
            const bool ok = alive[w] && e4[w].x == (W8 ? s[w] : (s[w] >> sub));
            const int sn = e4[w].y;
            const bool fin = ok && (unsigned)sn < nfin;
            log_put(fin, pos[w] | ((jn[w] & 15u) << 12) | ((unsigned)sn << 16));
            jn[w] += fin ? 1u : 0u;
            jmax |= jn[w];                     // (bit 4 or above: a 16th record at one position)
            pn[w] += 1u;
            alive[w] = ok && pn[w] < lim && (((unsigned)e4[w].w >> (nb[w] & 31u)) & 1u) != 0u;
            s[w] = sn;
            idx[w] = slot_of(e4[w].z, (unsigned)sn, nb[w]);
        }
        log_flush(false);
    }
    log_flush(true);
#ifdef PFAC_TRACE_BUILD
    if (a.dbg && blockIdx.x < 8 && lane == 0 && (threadIdx.x >> 6) == 0) {
        unsigned long long *acc = a.dbg + (size_t)blockIdx.x * 64 * 32 + 10;      // columns 10..14 of the block's row 0
        const unsigned long long tq_all = __builtin_amdgcn_s_memrealtime() - tq_t0;
        acc[0] += tq_front; acc[1] += tq_n; acc[2] += tq_all; acc[3] += 1; acc[4] += lc;
    }
    (void)tq_iter;
#endif
    if (__any(jmax > 15u) || lc > logcap) return ~0u;
    return lc;
}

// The tile's log -> its place in the record heap (4-byte records), in (position, length) order: the records of every
// position are counted (4-bit fields), the counts prefix-summed, and every log entry goes to base + prefix[position] + k.
__device__ __forceinline__ void dense2_scatter(const ScanArgs &a, unsigned char *aux, const unsigned *logg, unsigned cnt,
                                               unsigned long long base, int lane) {
    unsigned *cntw = reinterpret_cast<unsigned *>(aux + D2_CNT_OFF);
    unsigned *pref2 = reinterpret_cast<unsigned *>(aux + D2_PREF_OFF);            // u16 pairs
    const unsigned short *pref = reinterpret_cast<const unsigned short *>(aux + D2_PREF_OFF);
    auto nibsum = [](unsigned x) -> unsigned { return (((x & 0x0F0F0F0Fu) + ((x >> 4) & 0x0F0F0F0Fu)) * 0x01010101u) >> 24; };
    constexpr int UN = 4;                      // log words per lane per group
    constexpr int ER = 32;                     // a tile of up to ER x 64 records keeps its log words in registers between the two passes
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    reinterpret_cast<u32x4 *>(cntw)[lane] = zero4;
    reinterpret_cast<u32x4 *>(cntw)[lane + WAVE] = zero4;
    // (the log was written by other lanes of THIS wave: the workgroup-scope fence waits for their stores, and a CU's L1 is
    // coherent with the stores of its own waves -- an agent-scope release would write the whole L2 back, per tile)
    wave_lds_sync();
    // the tile's piece of the heap through a buffer descriptor: a scalar base, and what lies past the end of the record
    // array is dropped by the bounds check
    const unsigned long long room = base < a.out_cap ? a.out_cap - base : 0ull;
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(static_cast<unsigned *>(a.out) + base, 0,
                                                                         (int)((room < (unsigned long long)cnt ? (unsigned)room : cnt) * 4u), 0x00020000);
    auto count_one = [&](unsigned e) { atomicAdd(&cntw[(e & 0xFFFu) >> 3], 1u << ((e & 7u) * 4u)); };
    auto prefix = [&]() {
        wave_lds_sync();
        const u32x4 x0 = reinterpret_cast<const u32x4 *>(cntw)[2 * lane], x1 = reinterpret_cast<const u32x4 *>(cntw)[2 * lane + 1];
        unsigned sm[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { sm[k] = nibsum(x0[k]); sm[4 + k] = nibsum(x1[k]); }
        unsigned tot = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) tot += sm[k];
        unsigned run = wave_incl_scan(tot) - tot;
        u32x4 pw;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned lo = run; run += sm[2 * k];
            const unsigned hi = run; run += sm[2 * k + 1];
            pw[k] = lo | (hi << 16);
        }
        reinterpret_cast<u32x4 *>(pref2)[lane] = pw;
        wave_lds_sync();
    };
    auto place_one = [&](unsigned e) {
        const unsigned p = e & 0xFFFu, j = (e >> 12) & 15u, st = e >> 16;
        const unsigned x = cntw[p >> 3];
        const unsigned dest = (unsigned)pref[p >> 3] + nibsum(x & ((1u << ((p & 7u) * 4u)) - 1u)) + j;
        __builtin_amdgcn_raw_buffer_store_b32(p | (st << 12), ors, (int)(dest << 2), 0, 0);
    };
    if (cnt <= (unsigned)(ER * WAVE)) {
        const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned *>(logg), 0, (int)(cnt * 4u), 0x00020000);
        // the usual tile: every load of the log goes out before the first word is looked at -- the head of the log has left
        // the L2 by now (one memory latency per tile, not one per group of loads) -- and the words stay in registers for
        // the second pass
        unsigned e[ER];
#pragma unroll
        for (int g = 0; g < ER / UN; g++) {
            if ((unsigned)(g * UN * WAVE) < cnt) {
#pragma unroll
                for (int u = 0; u < UN; u++)      // (one lane offset, the group in the scalar offset; past the end of the log: 0)
                    e[g * UN + u] = __builtin_amdgcn_raw_buffer_load_b32(lrs, lane * 4, (g * UN + u) * WAVE * 4, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < ER / UN; g++) {
            if ((unsigned)(g * UN * WAVE) < cnt) {
#pragma unroll
                for (int u = 0; u < UN; u++)
                    if ((unsigned)((g * UN + u) * WAVE + lane) < cnt) count_one(e[g * UN + u]);
            }
        }
        prefix();
#ifdef PFAC_ABL_D2NOSCATTER                    // ablation builds only: the records never reach the heap
        cnt = 0;
#endif
#pragma unroll
        for (int g = 0; g < ER / UN; g++) {
            if ((unsigned)(g * UN * WAVE) < cnt) {
#pragma unroll
                for (int u = 0; u < UN; u++)
                    if ((unsigned)((g * UN + u) * WAVE + lane) < cnt) place_one(e[g * UN + u]);
            }
        }
        return;
    }
    for (unsigned i0 = 0; i0 < cnt; i0 += UN * WAVE) {
        unsigned e[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const unsigned i = i0 + (unsigned)(u * WAVE + lane);
            e[u] = i < cnt ? logg[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < UN; u++)
            if (i0 + (unsigned)(u * WAVE + lane) < cnt) count_one(e[u]);
    }
    prefix();
#ifdef PFAC_ABL_D2NOSCATTER
    cnt = 0;
#endif
    for (unsigned i0 = 0; i0 < cnt; i0 += UN * WAVE) {
        unsigned e[UN];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const unsigned i = i0 + (unsigned)(u * WAVE + lane);
            e[u] = i < cnt ? logg[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < UN; u++)
            if (i0 + (unsigned)(u * WAVE + lane) < cnt) place_one(e[u]);
    }
}

// Root test: 16-bit mask of the lane's 16 bytes that have an edge out of the root.
//   ROOT == 1: exactly one such byte value -> exact SWAR compare, flags gathered with v_dot4
//   ROOT == 0: one LDS lookup per byte in pre-shifted flag tables (byte k of a dword looks into table k).  The same lookup
//              answers a second question for free: bits 16..31 of the result = which of the 16 bytes can be the
//              SECOND byte of a pattern at all (the cheap half of the level-2 filter).
template <int ROOT>
__device__ __forceinline__ unsigned root_mask(const u32x4 w, const unsigned char *ftab, unsigned root_x4) {
    if (ROOT == 1) {
        unsigned nm[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned x = w[i] ^ root_x4;                            // zero byte <=> match
            nm[i] = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where the byte is NOT a match
        }
        unsigned lo = __builtin_amdgcn_udot4(nm[0], 0x08040201u, 0u, false);
        lo = __builtin_amdgcn_udot4(nm[1], 0x80402010u, lo, false);       // = 128 * (not-match bits 0..7)
        unsigned hi = __builtin_amdgcn_udot4(nm[2], 0x08040201u, 0u, false);
        hi = __builtin_amdgcn_udot4(nm[3], 0x80402010u, hi, false);
        return ~((lo >> 7) | (hi << 1)) & 0xFFFFu;
    } else {
        // four byte-wide tables, one per byte of a dword: table k holds  root flag << k | second-byte flag << (k + 4).
        // 256 bytes = 64 LDS words = one word per bank, so a wave's 64 random lookups never conflict (the 16-bit
        // tables, two words per bank, spent half their cycles on conflicts)
        const unsigned char *t8 = ftab;
        unsigned p = 0;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const unsigned d = w[g];
            const unsigned v = (unsigned)t8[d & 0xFFu] | (unsigned)t8[256 + ((d >> 8) & 0xFFu)] |
                               (unsigned)t8[512 + ((d >> 16) & 0xFFu)] | (unsigned)t8[768 + (d >> 24)];
            p |= v << (8 * g);
        }
        // p: byte g = dword g's flags, low nibble root, high nibble second-byte -> two 16-bit masks
        unsigned x = p & 0x0F0F0F0Fu, y = (p >> 4) & 0x0F0F0F0Fu;
        x = (x | (x >> 4)) & 0x00FF00FFu; y = (y | (y >> 4)) & 0x00FF00FFu;
        x = (x | (x >> 8)) & 0xFFFFu; y = (y | (y >> 8)) & 0xFFFFu;
        return x | (y << 16);
    }
}

// Bytes equal to x (replicated x4) among the lane's 32: bit b <=> byte b.
__device__ __forceinline__ unsigned eq_mask32(const u32x4 lo16, const u32x4 hi16, unsigned x4) {
    return root_mask<1>(lo16, nullptr, x4) | (root_mask<1>(hi16, nullptr, x4) << 16);
}

#ifdef PFAC_TRACE_BUILD
#define PFAC_STAMP(cond, slot) do { if (cond) tr[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PFAC_STAMP(cond, slot) do { } while (0)
#endif

// ---------------------------------------------------------------------------
// The scan kernel.  Workgroups share the read-only tables staged in LDS once; after that there is
// no workgroup barrier: compute waves pipeline  [loads of round r+1 in flight | scan round r |
// emit round r-2]  and meet the coordinator only through the LDS rings above.
#ifndef PFAC_SPARSE_FUSED_NW
#define PFAC_SPARSE_FUSED_NW 2
#endif
constexpr int MAX_WAVES_NW4 = 10;          // four walks per lane, staged in LDS: dense mode's buffers leave room for 9-10 waves per workgroup

template <bool TLDS, bool W8, int ROOT, bool FUSED, int NW, int NB, bool FOLD>
__device__ __forceinline__ void scan_body(const ScanArgs &a, unsigned char *smem, const ErrCh &err) {
    unsigned *hdr = reinterpret_cast<unsigned *>(smem + SH_HDR);
    int *s0 = reinterpret_cast<int *>(smem + SH_S0);
    unsigned char *ftab = smem + SH_FTAB;
    unsigned char *finl = smem + SH_FIN;
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction: keep it in an SGPR
    const int nc = (int)(blockDim.x >> 6) - 1;             // compute waves; wave nc coordinates

    // ---- the control header of the slot's NEXT scan (ticket counters, flags, heap cursor of its other buffer) is zeroed here,
    // spread over the whole grid: the next launch on the stream starts after this one has ended
    for (unsigned i = blockIdx.x * blockDim.x + tid; i < a.zero_vec; i += gridDim.x * blockDim.x)
        a.zero_next[i] = make_uint4(0u, 0u, 0u, 0u);
    // ---- once per workgroup: rings cleared, root row, root flag tables, (small) PHF tables -> LDS
    for (int i = tid; i < H_WORDS; i += blockDim.x) hdr[i] = 0;
    for (int i = tid; i < 256; i += blockDim.x) {
        const int v = a.s0[i];
        const bool sec2 = a.sec2[i] != 0;
        s0[i] = v;
        finl[i] = (unsigned)v < (unsigned)a.num_final ? (unsigned char)1 : (unsigned char)0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            ftab[k * 256 + i] = (unsigned char)((v >= 0 ? 1u << k : 0u) | (sec2 ? 1u << (k + 4) : 0u));
    }
    unsigned char *d1idx_l = smem + SH_D1IDX;
    int *d1_l = reinterpret_cast<int *>(smem + SH_D1);
    unsigned char *colmap_l = smem + SH_COLMAP;
    if (a.d1_rows > 0) {
        for (int i = tid; i < 256; i += blockDim.x) { d1idx_l[i] = a.d1idx[i]; colmap_l[i] = a.d1_colmap[i]; }
        // (only the columns of bytes some pattern has second; the last column of a row: no edge)
        for (int i = tid; i < a.d1_rows * a.d1_stride; i += blockDim.x) {
            const int row = i / a.d1_stride, c = i - row * a.d1_stride;
            d1_l[i] = c < a.d1_ncols ? a.d1[row * 256 + a.d1_colbyte[c]] : -1;
        }
    } else {
        for (int i = tid; i < 256; i += blockDim.x) { d1idx_l[i] = 0; colmap_l[i] = 0; }
    }
    if (a.d1_rows > 0)                         // (one more row, without edges: where dense2_tile sends the bytes that start no pattern)
        for (int i = tid; i < a.d1_stride; i += blockDim.x) d1_l[a.d1_rows * a.d1_stride + i] = -1;
    // root table of dense2_tile: final state of the byte's depth-1 state (0xFFFF: not final) | word offset of its dense row << 16
    const unsigned *t0_l = reinterpret_cast<const unsigned *>(smem + a.sh_t0);
    if (FUSED && NW == 4 && a.sh_t0)
        for (int i = tid; i < 256; i += blockDim.x) {
            const int v = a.s0[i];
            reinterpret_cast<unsigned *>(smem + a.sh_t0)[i] = v >= 0 ? (((unsigned)v < (unsigned)a.num_final ? (unsigned)v : 0xFFFFu) | ((unsigned)(a.d1idx[i] * a.d1_stride) << 16))
                                                                     : (0xFFFFu | ((unsigned)(a.d1_rows * a.d1_stride) << 16));
        }
    int2 *d1r2_l = reinterpret_cast<int2 *>(smem + SH_D1 + a.d1_lds_bytes);
    if (FUSED && a.d1_n2 > 0)
        for (int i = tid; i <= a.d1_n2; i += blockDim.x) {     // (one more entry, {0, no child}: where dense2_tile sends "no second state")
            const int2 e = i < a.d1_n2 ? a.d1r2[i] : make_int2(-a.rn_bias, 0);
            d1r2_l[i] = make_int2(e.x + a.rn_bias, e.y);
        }
    // FUSED without dense rows: r[] of the depth-1 states by root byte, in the (unused) dense-row region
    int *s0r_l = reinterpret_cast<int *>(smem + SH_D1);
    const bool have_s0r = FUSED && a.d1_rows == 0;
    if (have_s0r)
        for (int i = tid; i < 256; i += blockDim.x) {
            const int v = a.s0[i];
            s0r_l[i] = v >= 0 ? a.r[v >> (a.wbit - 8)] + a.rn_bias : 0;
        }
    const Dense1 d1 = {colmap_l, d1idx_l, d1_l, a.d1_rows > 0, (FUSED && a.d1_n2 > 0) ? d1r2_l : nullptr, have_s0r ? s0r_l : nullptr};
    const int sh_tab = SH_D1 + a.d1_lds_bytes;       // (the packed rows' r[] and LDS tables never coexist)
    const int *R = a.r;
    const int2 *T = a.T;
    if (TLDS) {
        int *lr = reinterpret_cast<int *>(smem + sh_tab);
        int2 *lt = reinterpret_cast<int2 *>(smem + sh_tab + ((a.r_words * 4 + 15) & ~15));
        for (int i = tid; i < a.r_words; i += blockDim.x) lr[i] = a.r[i];
        for (int i = tid; i < a.t_entries; i += blockDim.x) lt[i] = a.T[i];
        R = lr;
        T = lt;
    }
    // level-2 filter, lookup form: the 2-byte-prefix bitmap (all 256 rows, or the root byte's row when ROOT == 1)
    const unsigned char *bm2l = smem + a.sh_bm2;
    if (a.l2f_mode == 2) {
        const unsigned *src = reinterpret_cast<const unsigned *>(a.bm2 + (ROOT == 1 ? (a.root_byte & 0xFFu) * 32u : 0u));
        unsigned *dst = reinterpret_cast<unsigned *>(smem + a.sh_bm2);
        for (int i = tid; i < a.bm2_rows * 8; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();                           // the only workgroup barrier
#ifdef PFAC_TRACE_BUILD
    if (a.dbg && blockIdx.x < 8 && threadIdx.x == 0) a.dbg[((size_t)blockIdx.x * 64 + 1) * 32 + 15] = __builtin_amdgcn_s_memrealtime();
#endif

#ifdef PFAC_ABL_NOCOORD                        // ablation builds only: static tiles, no coordinator, counts dropped
    if (wave == nc) return;
#endif
    if (wave == nc) {
        // ================= coordinator =================
        __builtin_amdgcn_s_setprio(3);         // tiny, latency-critical instruction stream
        // batch tickets: the atomic is ISSUED one iteration before its result is needed, so its ~1.3 us
        // round trip never blocks the coordinator
#ifdef PFAC_ABL_STATIC                         // ablation builds only (tools/abn.sh): batches dealt round-robin, no atomic
        unsigned abl_seq = 0;
        auto ticket = [&]() -> unsigned { return (abl_seq++) * gridDim.x + blockIdx.x; };
#else
        auto ticket = [&]() -> unsigned {
            unsigned g = 0;
            if (lane == 0) g = atomicAdd(&a.ctl[(blockIdx.x % a.ticket_ways) * 64u], 1u) * a.ticket_ways + blockIdx.x % a.ticket_ways;
            return g;                          // valid in lane 0 (not waited for here)
        };
#endif
        auto publish_batch = [&](unsigned r, unsigned g_lane0) -> unsigned {   // ring entry of round r; returns batch id
            if (lane == 0) {
                lds_store(&hdr[H_ARRIVED + (r & 7)], 0u);
                lds_store(&hdr[H_BATCH + (r & 7)], g_lane0);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                lds_store(&hdr[H_EPOCH + (r & 7)], r + 1);
            }
            return __builtin_amdgcn_readfirstlane(g_lane0);
        };
        unsigned g[AHEAD];                     // batch ids of rounds r .. r+AHEAD-1 (published)
#pragma unroll
        for (int k = 0; k < AHEAD; k++) g[k] = publish_batch((unsigned)k, ticket());
        unsigned t_pending = ticket();         // for round AHEAD, published at the top of iteration 0
        // the heap: this workgroup's current chunk [ch_base, ch_base + ch_size), ch_used records of it taken, and the
        // chunk on order (the atomic was issued when the current one came into use; its value sits in lane 0)
        unsigned long long *cursor = reinterpret_cast<unsigned long long *>(a.ctl + CTL_CURSOR);
        auto order_chunk = [&]() -> unsigned long long {
            unsigned long long v = 0;
            if (lane == 0 && a.chunk) v = __hip_atomic_fetch_add(cursor, (unsigned long long)a.chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return v;                          // valid in lane 0 (not waited for here)
        };
        unsigned long long ch_base = 0, spare = order_chunk(), local_total = 0;
        unsigned ch_size = 0, ch_used = 0;
        const unsigned rec_pad = a.rec_bytes == 2 ? 7u : 0u;           // a run's allocation: its count rounded up to rec_pad + 1
        for (unsigned r = 0;; r++) {
            const unsigned g_cur = g[0];
            const unsigned long long first = (unsigned long long)g_cur * (unsigned)nc;
            if (first >= a.n_tiles) break;     // batch ids only grow: nothing left for this workgroup
            const unsigned g_new = publish_batch(r + AHEAD, t_pending);   // AHEAD rounds ahead of this iteration
            t_pending = ticket();                           // for round r+AHEAD+1
#ifdef PFAC_TRACE_BUILD
            const bool trace = a.dbg && blockIdx.x < 8 && r < 64 && lane == 0;
            unsigned long long *tr = a.dbg + ((size_t)blockIdx.x * 64 + (r & 63)) * 32;
#endif
            PFAC_STAMP(trace, 0);
            // ---- round r: wait for the counts of its tiles
            const unsigned long long left = a.n_tiles - first;
            const unsigned n_valid = left < (unsigned long long)nc ? (unsigned)left : (unsigned)nc;
            if (!lds_wait_eq(&hdr[H_ARRIVED + (r & 7)], n_valid, err, 4u)) break;
            PFAC_STAMP(trace, 1);
            // (bit 31 of a posted count: that tile is emitted at once and has taken its own space from the heap cursor)
            const unsigned c_raw = (unsigned)lane < n_valid ? hdr[H_CNT + (r & 7) * 16 + lane] : 0u;
            const unsigned c_all = c_raw & 0x7FFFFFFFu;
            const bool self_placed = (c_raw >> 31) != 0u;
            // 16-bit records: each run takes its count rounded up to 8 records, so that every run starts on a 16-byte
            // boundary (chunks and exact allocations are multiples of 8 records too) and leaves as whole 16-byte stores
            const unsigned c = self_placed ? 0u : (c_all + rec_pad) & ~rec_pad;
            const unsigned incl = wave_incl_scan(c);        // 15 tile counts of < 2^22 each
            const unsigned tot = bcast_last(incl);
            const unsigned excl = incl - c;
            // ---- place the tiles (lane c: the tile of compute wave c)
            unsigned long long wb;
            if (tot == 0) {
                wb = ch_base + ch_used;                     // nothing to place (any valid index will do)
            } else if (tot > a.chunk) {
                // larger than a chunk (dense matches, or a small record array): an allocation of exactly this size
                unsigned long long v = 0;
                if (lane == 0) v = __hip_atomic_fetch_add(cursor, (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
                wb = (((unsigned long long)hi << 32) | lo) + excl;
            } else if (ch_used + tot <= ch_size) {
                wb = ch_base + ch_used + excl;
                ch_used += tot;
            } else {
                // the batch continues in the spare chunk from the first tile that does not fit into this one
                const unsigned long long fits = __ballot(ch_used + incl <= ch_size);    // a prefix of the lanes
                const unsigned k = (unsigned)__popcll(fits);                            // first lane that moves (0..nc-1)
                const unsigned off = __builtin_amdgcn_readlane(excl, k);
                const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)spare), hi = __builtin_amdgcn_readfirstlane((unsigned)(spare >> 32));
                const unsigned long long nb = ((unsigned long long)hi << 32) | lo;
                wb = (unsigned)lane < k ? ch_base + ch_used + excl : nb + (excl - off);
                ch_base = nb;
                ch_size = a.chunk;
                ch_used = tot - off;
                spare = order_chunk();
            }
            const bool mute = (a.fault & 1u) && blockIdx.x == 1 && r == 1;   // test knob: the bases of this round never come
            if (lane < nc) {
                hdr[H_WBASE + (r & 7) * 32 + lane * 2] = (unsigned)wb;
                hdr[H_WBASE + (r & 7) * 32 + lane * 2 + 1] = (unsigned)(wb >> 32);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0 && !mute) lds_store(&hdr[H_READY + (r & 7)], r + 1);
            if ((unsigned)lane < n_valid && !self_placed) a.tile_index[first + (unsigned)lane] = wb | ((unsigned long long)c_all << TIX_CNT_SHIFT);
            // the matches (exact counts, self-placed tiles included): behind the bases, off the compute waves' path
            local_total += (rec_pad || __any(self_placed)) ? bcast_last(wave_incl_scan(c_all)) : tot;
#ifdef PFAC_TRACE_BUILD
            if (trace) { tr[2] = __builtin_amdgcn_s_memrealtime(); tr[3] = g_cur; }
#endif
#pragma unroll
            for (int k = 0; k + 1 < AHEAD; k++) g[k] = g[k + 1];
            g[AHEAD - 1] = g_new;
        }
        // every count of this workgroup has been posted by now: matches, and how many tiles were denser than the sparse
        // staging capacity (the host switches staging mode on it)
        if (lane == 0) {
            if (local_total) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(a.ctl + CTL_TOTAL), local_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned ovf = lds_load(&hdr[H_OVF]);
            if (ovf) __hip_atomic_fetch_add(&a.ctl[CTL_OVF], ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned ovf2 = lds_load(&hdr[H_OVF2]);
            if (ovf2) __hip_atomic_fetch_add(&a.ctl[CTL_OVF2], ovf2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }

    // ================= compute waves =================
    unsigned char *tile = smem + a.shared_bytes + wave * a.pw_bytes;
    unsigned short *q = reinterpret_cast<unsigned short *>(tile + WTILE + a.halo);
    const bool d2 = NW == 4 && FUSED && a.dense2 != 0;         // dense mode, second form (dense2_tile); its LDS carve differs
    unsigned char *aux = tile + WTILE + a.halo;
    unsigned *stage0 = reinterpret_cast<unsigned *>(aux + QCAP * 2);        // (d2: never written, stage_cap is 0)
    unsigned *d2log = d2 ? a.d2log + ((size_t)blockIdx.x * (unsigned)nc + (unsigned)wave) * a.d2log_cap : nullptr;
    const bool root_final = ROOT == 1 && (unsigned)a.root_state < (unsigned)a.num_final;

    // prefetch registers: the wave's 4 KiB + halo, LOAD_DEPTH tiles ahead of the one being scanned (set A / set B)
    u32x4 wA[SUBS], wB[SUBS];
    u32x4 hA = {0u, 0u, 0u, 0u}, hB = {0u, 0u, 0u, 0u};
    auto issue_loads = [&](unsigned long long tt, u32x4 (&w)[SUBS], u32x4 &hw) {
        const unsigned long long tb = tt * WTILE;
        const unsigned long long remain = a.n_avail - tb;
        const unsigned lm = remain < (unsigned long long)(WTILE + a.halo) ? (unsigned)remain : (unsigned)(WTILE + a.halo);
        // the descriptor covers whole 16-B units only: every dword of a load is fully inside or reads as 0
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<unsigned char *>(a.in + tb), 0, (int)(lm & ~15u), 0x00020000);
#pragma unroll
        for (int j = 0; j < SUBS; j++) w[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, j * SUB + lane * 16, 0, LOAD_AUX);
        if (lane * 16 < a.halo) hw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, WTILE + lane * 16, 0, 0);
    };
    // this wave's tile of round rr; false: there is none (the input is used up) or the ring timed out.
    // Tile numbers are wave-uniform: as scalars they make the buffer descriptor of the tile loads a scalar too
    // (a descriptor in VGPRs costs a readfirstlane "waterfall" loop around every load)
    auto probe = [&](unsigned rr, unsigned long long &tt) -> bool {
#ifdef PFAC_ABL_NOCOORD
        tt = ((unsigned long long)rr * gridDim.x + blockIdx.x) * (unsigned)nc + (unsigned)wave;
        return tt < a.n_tiles;
#endif
        if (!lds_wait_eq(&hdr[H_EPOCH + (rr & 7)], rr + 1, err, 16u)) return false;
        tt = (unsigned long long)__builtin_amdgcn_readfirstlane(hdr[H_BATCH + (rr & 7)]) * (unsigned)nc + (unsigned)wave;
        return tt < a.n_tiles;
    };
    // first record index of this wave's tile of round rr (computed by the coordinator)
    auto record_base = [&](unsigned rr, unsigned long long &base) -> bool {
        if (!lds_wait_eq(&hdr[H_READY + (rr & 7)], rr + 1, err, 8u)) return false;
        // (every lane reads the same words: tell the compiler, so the record addresses get a scalar base)
        const unsigned blo = __builtin_amdgcn_readfirstlane(hdr[H_WBASE + (rr & 7) * 32 + wave * 2]);
        const unsigned bhi = __builtin_amdgcn_readfirstlane(hdr[H_WBASE + (rr & 7) * 32 + wave * 2 + 1]);
        base = ((unsigned long long)bhi << 32) | blo;
        return true;
    };

    unsigned r = 0;
    unsigned long long t = 0, t_n1 = 0;        // tiles of rounds r and (LOAD_DEPTH == 2) r+1
    bool have_n1 = false;
    if (!probe(0, t)) return;
    issue_loads(t, wA, hA);
    if (LOAD_DEPTH == 2) {
        have_n1 = probe(1, t_n1);
        if (have_n1) issue_loads(t_n1, wB, hB);
    }

    // pend_have[k]: the tile scanned k+1 rounds ago still sits in its staging buffer (pend_cnt[k] records)
    // NB == 3: the three-buffer kernels (a.nbuf == 3); NB == 2: two buffers, or one (dense mode)
    constexpr int LAG_MAX = NB - 1;
    const unsigned nbuf = NB == 3 ? 3u : a.nbuf;
    const unsigned lag = NB == 3 ? 2u : a.nbuf - 1u;   // rounds between a tile's scan and its emission (0: dense mode)
    bool pend_have[LAG_MAX];
    unsigned pend_cnt[LAG_MAX], buf = 0;       // buf: staging buffer of the current round, (r % nbuf)
#pragma unroll
    for (int k = 0; k < LAG_MAX; k++) { pend_have[k] = false; pend_cnt[k] = 0; }

    // One round: w / hw hold this round's tile; they are refilled with the tile LOAD_DEPTH rounds ahead as soon as
    // their bytes sit in LDS.  Returns false after the wave's last tile.
    auto round_body = [&](u32x4 (&w)[SUBS], u32x4 &hw) -> bool {
        const unsigned long long tile_base = t * WTILE;
        const unsigned long long remain = a.n_avail - tile_base;           // > 0
        const unsigned lim = remain < (unsigned long long)(WTILE + a.halo) ? (unsigned)remain : (unsigned)(WTILE + a.halo);

#ifdef PFAC_TRACE_BUILD
        const bool trace = a.dbg && blockIdx.x < 8 && r < 64 && lane == 0 && wave == 0;
        unsigned long long *tr = a.dbg + ((size_t)blockIdx.x * 64 + (r & 63)) * 32;
#endif
        PFAC_STAMP(trace, 4);
        // ---- registers -> LDS (tile + halo), then start the loads of the tile LOAD_DEPTH rounds ahead right away
#ifndef PFAC_ABL_NOLDSCOPY                     // ablation builds only: the tile never reaches LDS (wrong masks)
        // (case-insensitive scans fold here, and in the tail patch below: everything that looks at input bytes afterwards
        // reads this LDS copy, and the caller's buffer is only ever loaded.  FOLD is a template parameter: the exact kernels
        // hold no trace of it -- a runtime flag around this block came out of its A/B call 1 % slower with the fold OFF on
        // the headline workload)
        if (FOLD) {
#pragma unroll
            for (int j = 0; j < SUBS; j++) w[j] = fold4(w[j]);
            hw = fold4(hw);
        }
#pragma unroll
        for (int j = 0; j < SUBS; j++) *reinterpret_cast<u32x4 *>(tile + j * SUB + lane * 16) = w[j];
        if (lane * 16 < a.halo) *reinterpret_cast<u32x4 *>(tile + WTILE + lane * 16) = hw;
#else
        asm volatile("" :: "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(hw));
#endif
        if (lim & 15u) {                       // ragged end of the input (last tile only): patch the tail bytes
            wave_lds_sync();
            if (lane < (int)(lim & 15u)) {
                const unsigned char b = a.in[tile_base + (lim & ~15u) + lane];
                tile[(lim & ~15u) + lane] = FOLD ? pfac_fold_byte(b) : b;
            }
        }
        wave_lds_sync();
        PFAC_STAMP(trace, 5);
        unsigned long long t_far = 0;
        const bool more_far = (LOAD_DEPTH == 1 || have_n1) && probe(r + LOAD_DEPTH, t_far);
        if (more_far) issue_loads(t_far, w, hw);
        PFAC_STAMP(trace && r > 0, 10);
        // ---- emit the tile of `lag` rounds ago: its bases came when that round's last count was in (a tile without
        // records has nothing to wait for: the coordinator stores the tile index).  Its buffer is the one after the
        // current round's, cyclically.
        auto emit_pending = [&](bool have, unsigned n_rec) {
            if (have && n_rec != 0) {
                unsigned long long base = 0;
                const bool okb = record_base(r - lag, base);
                PFAC_STAMP(trace, 9);
                if (okb) copy_out<!TLDS>(a, stage0 + (buf + 1u == nbuf ? 0u : buf + 1u) * a.stage_cap, n_rec, base, lane);
            }
        };
        if (NB == 3) emit_pending(pend_have[LAG_MAX - 1], pend_cnt[LAG_MAX - 1]);      // stores right behind the loads
        PFAC_STAMP(trace && r > 0, 11);

        // ---- root test -> 32-bit survivor mask per lane per half-tile; level-2 filter -> which of them are kept
        // (yield a record or need a walk) and which of those are deep (need the walk)
        unsigned keep[MSUBS] = {0u, 0u}, deep[MSUBS] = {0u, 0u};
        unsigned *stage = stage0 + buf * a.stage_cap;
        // dense mode on fused tables with packed dense rows: no classification, no rounds (dense2_tile); a tile it gives
        // up on (log full, > 15 patterns at one offset) goes the classic way below
        unsigned d2cnt = ~0u;
        if (NW == 4 && FUSED) {
            if (d2) {
                const unsigned long long own = a.n_owned - tile_base;
                d2cnt = dense2_tile<W8>(a, tile, t0_l, d1, aux, d2log, lane, lim, own < (unsigned long long)WTILE ? (unsigned)own : (unsigned)WTILE);
            }
        }
        const bool d2done = d2cnt != ~0u;
        PFAC_STAMP(trace && r > 0 && d2, 12);
        if (!d2done) {
#pragma unroll
        for (int j = 0; j < MSUBS; j++) {
            const unsigned off = j * MSUB + lane * MLANE;
            const u32x4 lo16 = *reinterpret_cast<const u32x4 *>(tile + off);
            const u32x4 hi16 = *reinterpret_cast<const u32x4 *>(tile + off + 16);
#ifdef PFAC_ABL_NOROOT                         // ablation builds only: no root test (nothing survives)
            const unsigned rlo = (lo16[0] == 0x12345678u), rhi = (hi16[0] == 0x12345678u);
#else
            const unsigned rlo = root_mask<ROOT>(lo16, ftab, a.root_byte), rhi = root_mask<ROOT>(hi16, ftab, a.root_byte);
#endif
            const unsigned raw = (rlo & 0xFFFFu) | (rhi << 16);
#ifdef PFAC_TRACE_BUILD
            asm volatile("" :: "v"(raw));
            PFAC_STAMP(trace && r > 0, j == 0 ? 12 : 14);
#endif
            unsigned m1 = raw;
            if (tile_base + WTILE > a.n_owned) {   // last tile only: offsets at or past n_owned start no walk
                const unsigned long long g = tile_base + off;
                if (g + MLANE > a.n_owned) m1 = g >= a.n_owned ? 0u : (m1 & ((1u << (unsigned)(a.n_owned - g)) - 1u));
            }
            if (a.l2f_mode == 0) {
                keep[j] = m1;
                deep[j] = m1;
            } else if (ROOT == 1 && a.l2f_mode == 1) {
                // bit-parallel: deep <=> the NEXT byte is a child byte of the depth-1 state (byte 32 = the first byte of
                // the next lane's run, or of the halo)
                unsigned nextc = 0;
                if (a.n_child > 0) {
                    const unsigned nx = *reinterpret_cast<const unsigned *>(tile + off + 32);
                    unsigned ec = a.child0 == a.root_byte ? raw : eq_mask32(lo16, hi16, a.child0);
                    unsigned e32 = ((nx ^ a.child0) & 0xFFu) == 0u ? 1u : 0u;
                    if (a.n_child > 1) {
                        ec |= a.child1 == a.root_byte ? raw : eq_mask32(lo16, hi16, a.child1);
                        e32 |= ((nx ^ a.child1) & 0xFFu) == 0u ? 1u : 0u;
                    }
                    nextc = (ec >> 1) | (e32 << 31);
                }
                deep[j] = m1 & nextc;
                keep[j] = root_final ? m1 : deep[j];
            } else {
                // one lookup per survivor in the 2-byte-prefix bitmap (and, for a multi-edge root, in the
                // depth-1-state-is-final table).  Per-lane loop, up to L2F_UNROLL survivors per trip: their lookups are
                // independent chains of two LDS round trips, so a trip costs one chain, not four.
                unsigned dm = 0, fm = 0;
                const unsigned *t32 = reinterpret_cast<const unsigned *>(tile);
                unsigned cand = m1;
                if (ROOT != 1 && a.sec_filter) {
                    // multi-edge root without 1-byte patterns: only survivors whose NEXT byte can be a second byte at
                    // all are looked up (flags of bytes 1..31 from the root test's own lookups, byte 32 = one more)
                    const unsigned nx = *reinterpret_cast<const unsigned *>(tile + off + 32);
                    const unsigned s32 = ((unsigned)ftab[nx & 0xFFu] >> 4) & 1u;
                    cand = m1 & ((((rlo >> 16) | (rhi & 0xFFFF0000u)) >> 1) | (s32 << 31));
                }
#ifdef PFAC_ABL_NOCLASS                        // ablation builds only: no survivor is looked up (no records)
                cand = 0;
#endif
                if (ROOT != 1 && a.l2f_mode == 3) {
                    // dense pair matrix (most flagged first bytes are followed by most flagged second bytes in the
                    // trie): the per-survivor bitmap lookup -- a serial, per-lane chain of LDS round trips -- would drop
                    // few of these, so they all go to the walk, whose dense depth-1 row IS the pair lookup, 64 lanes wide
                    dm = cand;
                    cand = 0;
                }
                for (unsigned mm = cand; mm;) {
                    unsigned b[L2F_UNROLL], win[L2F_UNROLL], v[L2F_UNROLL], fin[L2F_UNROLL];
                    bool on[L2F_UNROLL];
#pragma unroll
                    for (int u = 0; u < L2F_UNROLL; u++) {
                        on[u] = mm != 0u;
                        b[u] = on[u] ? (unsigned)__ffs(mm) - 1u : 0u;
                        mm &= mm - 1u;                              // (0 stays 0)
                        const unsigned p = off + b[u];
                        const unsigned lo = t32[p >> 2], hi = t32[(p >> 2) + 1];
                        win[u] = __builtin_amdgcn_alignbyte(hi, lo, p & 3u);   // bytes p .. p+3
                    }
#pragma unroll
                    for (int u = 0; u < L2F_UNROLL; u++) {
                        const unsigned b0 = win[u] & 0xFFu, b1 = (win[u] >> 8) & 0xFFu;
                        v[u] = bm2l[(ROOT == 1 ? 0u : b0 * 32u) + (b1 >> 3)];
                        fin[u] = ROOT == 1 ? 0u : (unsigned)finl[b0];
                    }
#pragma unroll
                    for (int u = 0; u < L2F_UNROLL; u++) {
                        const unsigned b1 = (win[u] >> 8) & 0xFFu;
                        dm |= on[u] ? ((v[u] >> (b1 & 7u)) & 1u) << b[u] : 0u;
                        fm |= on[u] ? fin[u] << b[u] : 0u;
                    }
                }
                deep[j] = dm;
                keep[j] = dm | (ROOT == 1 ? (root_final ? m1 : 0u) : fm);
            }
#ifdef PFAC_TRACE_BUILD
            asm volatile("" :: "v"(keep[j]), "v"(deep[j]));
            PFAC_STAMP(trace && r > 0 && j == 0, 13);
#endif
        }
        }

#ifdef PFAC_ABL_NOKEEP                         // ablation builds only: survivors classified, then dropped (no records)
        asm volatile("" :: "v"(keep[0]), "v"(keep[1]), "v"(deep[0]), "v"(deep[1]));
        keep[0] = keep[1] = deep[0] = deep[1] = 0;
#endif
        PFAC_STAMP(trace, 6);
        // ---- compact + walk once; records staged in LDS buffer `buf`; post the count
        // (a tile nothing survives in -- most tiles of a sparse pattern set -- goes straight to posting its zero)
        const unsigned long long cnt = d2done ? (unsigned long long)d2cnt : !__any((keep[0] | keep[1]) != 0u) ? 0ull :
            tile_pass<W8, false, NW, FUSED, ROOT>(a, tile, s0, d1, R, T, q, stage, keep, deep, lane, lim, tile_base, 0);
        PFAC_STAMP(trace, 7);
#ifdef PFAC_TRACE_BUILD
        if (a.dbg && blockIdx.x < 8 && r < 64 && lane == 0) tr[16 + wave] = __builtin_amdgcn_s_memrealtime();
#endif
        const bool overflow = cnt > a.stage_cap;
        const bool now = overflow || nbuf == 1;          // this tile is emitted right away (needs its base at once)
        unsigned arrival = 0;
#ifdef PFAC_ABL_NOCOORD
        if (false)
#endif
        if (lane == 0) {
            hdr[H_CNT + (r & 7) * 16 + wave] = (unsigned)cnt | ((now && cnt != 0) ? 0x80000000u : 0u);
            if (cnt > a.small_cap) {
                atomicAdd(&hdr[H_OVF2], 1u);
                if (cnt > a.sparse_cap) atomicAdd(&hdr[H_OVF], 1u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            arrival = atomicAdd(&hdr[H_ARRIVED + (r & 7)], 1u);
        }
        // The SIMD arbitrates VALU issue by priority, then age, so the youngest wave of each SIMD falls
        // behind and everybody ends up waiting for it.  Waves that arrived in the later half of this round
        // run the next one at raised priority: the laggards catch up, the round time approaches the mean.
        if (__builtin_amdgcn_readfirstlane(arrival) * 2u >= (unsigned)nc) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);

        if (now && cnt != 0) {
            // A tile that leaves at once waits for nobody: it takes exactly its records from the heap cursor itself (one
            // device atomic per tile -- these are the dense tiles, tens of microseconds each) and writes its own index
            // word; the coordinator only adds its count to the total.  (16-bit records: a multiple of 8 records, like
            // every allocation of the heap -- the runs placed after it stay on 16-byte boundaries.)
            const unsigned long long take = a.rec_bytes == 2 ? (cnt + 7ull) & ~7ull : cnt;
            unsigned long long v = 0;
            if (lane == 0)
                v = __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(a.ctl + CTL_CURSOR), take,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long base = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
                                            __builtin_amdgcn_readfirstlane((unsigned)v);
            if (lane == 0) a.tile_index[t] = base | ((unsigned long long)cnt << TIX_CNT_SHIFT);
            PFAC_STAMP(trace && r > 0 && d2, 13);
            if (NW == 4 && FUSED && d2done) {
                dense2_scatter(a, aux, d2log, (unsigned)cnt, base, lane);
                PFAC_STAMP(trace && r > 0, 14);
            }
            else if (overflow)
                // staging overflowed (or the automaton is too large for packed staging): walk the tile again,
                // while its bytes are still in LDS, writing straight to global memory
                tile_pass<W8, true, NW, FUSED, ROOT>(a, tile, s0, d1, R, T, q, stage, keep, deep, lane, lim, tile_base, base);
            else
                copy_out<!TLDS>(a, stage, (unsigned)cnt, base, lane);   // dense mode: staged, emitted at once
        }
        if (NB == 2) emit_pending(pend_have[0], pend_cnt[0]);
        PFAC_STAMP(trace, 8);
        if (NB == 3) { pend_have[LAG_MAX - 1] = pend_have[0]; pend_cnt[LAG_MAX - 1] = pend_cnt[0]; }
        pend_have[0] = !now; pend_cnt[0] = (unsigned)cnt;
        buf = buf + 1u >= nbuf ? 0u : buf + 1u;
        if (LOAD_DEPTH == 1) {
            if (!more_far) return false;
            t = t_far;
        } else {
            if (!have_n1) return false;
            t = t_n1;
            t_n1 = t_far;
            have_n1 = more_far;
        }
        r++;
        return true;
    };
    for (;;) {
        if (!round_body(wA, hA)) break;
        if (LOAD_DEPTH == 2 && !round_body(wB, hB)) break;
    }
    // drain: the tiles of the last `lag` rounds (pend_have[k]: round r - k, staged in buffer (r - k) % nbuf)
#pragma unroll
    for (int k = LAG_MAX - 1; k >= 0; k--) {
        if ((unsigned)k < lag && pend_have[k] && pend_cnt[k] != 0) {
            unsigned long long base = 0;
            if (record_base(r - (unsigned)k, base))
                copy_out<!TLDS>(a, stage0 + ((buf + nbuf - 1u - (unsigned)k) % nbuf) * a.stage_cap, pend_cnt[k], base, lane);
        }
    }
}

template <bool TLDS, bool W8, int ROOT, bool FUSED, int NW, int NB = 2, bool FOLD = false>
__global__ __launch_bounds__(WAVE * MAX_WAVES_PER_BLOCK) void pfac_scan_kernel(ScanArgs a) {
    static_assert(NB == 2 || (NB == 3 && NW <= 3), "three staging buffers: the sparse-mode kernels (dense mode has one)");
    static_assert(!(TLDS && FUSED), "the fused table is for tables gathered through L2");
    static_assert(NW == (TLDS ? 1 : 2) || (FUSED && (NW == 3 || NW == 4)), "walks per lane: 1 (LDS tables), 2 (L2 tables), 3 (L2, fused), 4 (L2, fused, dense matches)");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ErrCh err = {&a.ctl[CTL_ERR], a.spin_max};
#ifdef PFAC_TRACE_BUILD                        // column 15 of a traced workgroup's rows 0 / 1 / 2: entry, tables staged, last wave out
    if (a.dbg && blockIdx.x < 8 && threadIdx.x == 0) a.dbg[((size_t)blockIdx.x * 64 + 0) * 32 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
    // the kernel's start time, by its own clock: the earliest entry among the first workgroups (no return value: the lane
    // does not wait for the atomic)
    if (blockIdx.x < T0_GROUPS && threadIdx.x == 0)
        (void)__hip_atomic_fetch_max(reinterpret_cast<unsigned long long *>(a.ctl + CTL_T0), ~__builtin_amdgcn_s_memrealtime(),
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    scan_body<TLDS, W8, ROOT, FUSED, NW, NB, FOLD>(a, smem, err);
    // ---- leaving: the last wave of the workgroup counts the workgroup out; the last workgroup of the grid copies
    // the error flags and the dense-tile count from the control header (device memory) to the host-visible result
    // words with plain stores.  Every wave comes through here, whichever way it left the loop.
    unsigned *hdr = reinterpret_cast<unsigned *>(smem + SH_HDR);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's flag atomics have been performed
        const unsigned left = atomicAdd(&hdr[H_EXIT], 1u);
        if (left + 1 == (blockDim.x >> 6)) {
#ifdef PFAC_TRACE_BUILD
            if (a.dbg && blockIdx.x < 8) a.dbg[((size_t)blockIdx.x * 64 + 2) * 32 + 15] = __builtin_amdgcn_s_memrealtime();
#endif
            // Relaxed: the last workgroup reads nothing but words that every workgroup changed with device-scope atomics, and
            // each wave waited for its own (vmcnt above) before it was counted out, so they are performed when CTL_DONE
            // reaches the grid.  Records, tile index and the next control header are read only after the kernel (its end
            // releases them).  An acq_rel here wrote the XCD's L2 back at every workgroup's exit (buffer_wbl2): with the
            // records of the last rounds dirty in it, several microseconds on the path of the last workgroups to leave.
            const unsigned done = __hip_atomic_fetch_add(&a.ctl[CTL_DONE], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (done + 1 == gridDim.x) {
                const unsigned long long tot = __hip_atomic_load(reinterpret_cast<unsigned long long *>(a.ctl + CTL_TOTAL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long cur = __hip_atomic_load(reinterpret_cast<unsigned long long *>(a.ctl + CTL_CURSOR), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a.res[0] = (unsigned)tot; a.res[1] = (unsigned)(tot >> 32);
                a.res[2] = __hip_atomic_load(&a.ctl[CTL_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a.res[3] = __hip_atomic_load(&a.ctl[CTL_OVF], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a.res[4] = (unsigned)cur; a.res[5] = (unsigned)(cur >> 32);
                a.res[6] = __hip_atomic_load(&a.ctl[CTL_OVF2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // first workgroup in -> last workgroup out, then the completion word: ONE wave, once per launch, releases
                // the result words above to the host (not the per-workgroup write-back that the comment above is about)
                const unsigned long long t0 = ~__hip_atomic_load(reinterpret_cast<unsigned long long *>(a.ctl + CTL_T0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
                a.res[RES_T0] = (unsigned)t0; a.res[RES_T0 + 1] = (unsigned)(t0 >> 32);
                a.res[RES_T1] = (unsigned)t1; a.res[RES_T1 + 1] = (unsigned)(t1 >> 32);
                __hip_atomic_store(&a.res[RES_DONE], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// small service kernels

// blob (int32 image, pfac.h) -> device layout {s0[256] | r[max_row] | pad | T[ht_size] int2 | idmap}
// (*bad is set when the image would send a walk outside the tables: a row displacement outside the hash table, a root
// or next state that is no state -- the fused walk indexes with these values unchecked; its slot array is padded to
// max(r) + width entries, see pfac_fuse_kernel)
__global__ void pfac_repack_kernel(const int *blob, int *s0, int *r, int2 *T, int *idmap, int max_row, int ht_size,
                                   int num_final, int state_num, int width, int *bad) {
    const int *b_s0 = blob + PFAC_BLOB_HEADER_WORDS;
    const int *b_r = b_s0 + 256;
    const int *b_HT = b_r + max_row;
    const int *b_val = b_HT + ht_size;
    const int *b_id = b_val + ht_size;
    const int stride = gridDim.x * blockDim.x;
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = true;
    for (int i = i0; i < 256; i += stride) { s0[i] = b_s0[i]; ok = ok && b_s0[i] >= -1 && b_s0[i] < state_num; }
    for (int i = i0; i < max_row; i += stride) { r[i] = b_r[i]; ok = ok && b_r[i] > -width && b_r[i] < ht_size; }
    for (int i = i0; i < ht_size; i += stride) {
        T[i] = make_int2(b_HT[i], b_val[i]);
        ok = ok && (b_HT[i] < 0 || (b_val[i] >= -1 && b_val[i] < state_num));     // (an unowned slot's value is never used)
    }
    for (int i = i0; i < num_final; i += stride) idmap[i] = b_id[i];
    if (!ok) *bad = 1;
}

// Child mask of a state (the fused walk's prefilter): bit (c & 31) set iff the state has an edge on byte c.
__device__ __forceinline__ unsigned child_mask32(const int *r, const int2 *T, int wbit, int ht_size, int max_row, int state) {
    unsigned m = 0;
    if (state < 0) return 0u;
    for (int c = 0; c < 256; c++) {
        const int key = (state << 8) | c;
        const int row = key >> wbit;
        if (row >= max_row) continue;
        const int idx = r[row] + (key & ((1 << wbit) - 1));
        if ((unsigned)idx < (unsigned)ht_size) {
            const int2 e = T[idx];
            if (e.x == row && e.y >= 0) m |= 1u << (c & 31);
        }
    }
    return m;
}

// Fused slots for tables gathered through L2 (PHF width >= 256): T4[i] = {owner row, next state, r[row of next], 0}.
// (slots [lo, hi) with lo <= min(r), hi >= max(r) + width: the table image holds [0, ht_size) -- displacements may be
// negative and the image ends at its last used slot -- but the fused walk indexes unchecked; the slots outside the
// image are empty ones.  T4 points at slot 0.)
__global__ void pfac_fuse_kernel(const int2 *T, const int *r, int wbit, int ht_size, int max_row, int4 *T4, int lo, int hi) {
    const int stride = gridDim.x * blockDim.x;
    for (int i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride) {
        const int2 e = (i >= 0 && i < ht_size) ? T[i] : make_int2(-1, -1);
        int rn = -1;                           // (.z: r[row of the next state], biased like every fused index: slot - lo)
        bool have = false;
        if (e.y >= 0) {
            const int row = e.y >> (wbit - 8);
            if (row < max_row) { rn = r[row]; have = true; }
        }
        // .w: the child mask of the next state -- what lets the walk drop a walker without the gather that would
        // (only owned slots are ever selected, so an unowned slot's mask is never used)
        T4[i] = make_int4(e.x, e.y, have ? rn - lo : 0, e.x >= 0 ? (int)child_mask32(r, T, wbit, ht_size, max_row, e.y) : 0);
    }
}

// Dense rows of the depth-1 states: row f, column c = lookup(state d1state[f], byte c) through the PHF.
__global__ void pfac_build_d1_kernel(const int *d1state, const int *r, const int2 *T, int wbit, int ht_size, int *d1) {
    const int st = d1state[blockIdx.x];
    const int c = threadIdx.x;
    const int key = (st << 8) | c;
    const int row = key >> wbit;
    const int idx = r[row] + (key & ((1 << wbit) - 1));
    int nx = -1;
    if ((unsigned)idx < (unsigned)ht_size) {
        const int2 e = T[idx];
        if (e.x == row) nx = e.y;
    }
    d1[blockIdx.x * 256 + c] = nx;
}

// FUSED: pack the dense rows in place -- entry = state | k << 20 with r2[k] = {r[row of that state], its child mask};
// *counter hands out k.
__global__ void pfac_pack_d1_kernel(int *d1, int n_entries, const int *r, const int2 *T, int wbit, int ht_size, int max_row, int2 *r2, int *counter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const int nx = d1[i];
    if (nx < 0) return;
    const int k = atomicAdd(counter, 1);
    const int row = nx >> (wbit - 8);
    r2[k] = make_int2(row < max_row ? r[row] : -1, (int)child_mask32(r, T, wbit, ht_size, max_row, nx));
    d1[i] = nx | (k << D1_STATE_BITS);
}

// 2-byte-prefix bitmap: bit (b0 << 8 | b1) set iff the root has an edge on b0 and that state one on b1 (the level-2
// filter of the scan).  One block per b0, one thread per b1; a wave's ballot is 8 bytes of the row.
__global__ void pfac_build_bm2_kernel(const int *s0, const int *r, const int2 *T, int wbit, int ht_size, unsigned long long *bm2) {
    const int st = s0[blockIdx.x];
    const int c = threadIdx.x;
    int nx = -1;
    if (st >= 0) {
        const int key = (st << 8) | c;
        const int row = key >> wbit;
        const int idx = r[row] + (key & ((1 << wbit) - 1));
        if ((unsigned)idx < (unsigned)ht_size) {
            const int2 e = T[idx];
            if (e.x == row) nx = e.y;
        }
    }
    const unsigned long long bits = __ballot(nx >= 0);
    if ((c & (WAVE - 1)) == 0) bm2[blockIdx.x * 4 + (c >> 6)] = bits;
}

__device__ __forceinline__ unsigned long long match_hash(unsigned long long pos, unsigned id) {
    unsigned long long x = (pos + 1) * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)id * 0xC2B2AE3D27D4EB4Full);
    x ^= x >> 29;
    return x * 0xBF58476D1CE4E5B9ull;
}

// Records are read through the tile index (the heap has gaps): tile t holds tix[t] >> 40 records from index
// tix[t] & TIX_BASE_MASK on; records past the capacity of the array were never written.
template <int BYTES>
__device__ __forceinline__ void heap_record(const void *rec, unsigned long long i, unsigned long long tile, unsigned &pos, unsigned &state) {
    if (BYTES == 2) {
        const unsigned w = static_cast<const unsigned short *>(rec)[i];
        pos = (unsigned)(tile * WTILE) + (w & 0xFFFu);
        state = w >> 12;
    } else if (BYTES == 4) {
        const unsigned w = static_cast<const unsigned *>(rec)[i];
        pos = (unsigned)(tile * WTILE) + (w & 0xFFFu);
        state = w >> 12;
    } else {
        const pfac_record r = static_cast<const pfac_record *>(rec)[i];
        pos = r.pos;
        state = r.state;
    }
}

// Order-independent checksum of all records: one wave per tile at a time.
template <int BYTES>
__global__ void pfac_checksum_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles,
                                     unsigned long long cap, unsigned long long base, const int *idmap, unsigned long long *out) {
    unsigned long long sum = 0;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wstride = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n_tiles; t += wstride) {
        const unsigned long long e = tix[t], lo = e & TIX_BASE_MASK;
        const unsigned cnt = (unsigned)(e >> TIX_CNT_SHIFT);
        for (unsigned i = (unsigned)lane; i < cnt && lo + i < cap; i += WAVE) {
            unsigned pos, st;
            heap_record<BYTES>(rec, lo + i, t, pos, st);
            sum += match_hash(base + pos, (unsigned)idmap[st]);
        }
    }
    sum = wave_sum64(sum);
    if (lane == 0) atomicAdd(out, sum);
}

// Histogram of the final states (pfac_records_count_states / pfac_selection_count_states): the checksum's walk over
// the heap (one wave per tile at a time), or over a flat pfac_record array in chunks of 64, reduced ON CHIP first.
// A workgroup keeps 32-bit partial counts in LDS and adds the non-zero ones to the 64-bit counters in memory once, at
// its end.  Two LDS tables:
//   DIRECT  n_states <= bins: lds[s] is the partial of state s.
//   cache   2 words per slot {tag, count}, slot = count_slot_of(state): the first state that reaches an empty slot
//           claims it (tag = state + 1, by compare-and-swap) and counts there from then on; a state whose slot belongs
//           to another one adds to memory at once.  Hot states are seen early, so the hot traffic stays in LDS.
// Why a 32-bit partial cannot wrap: a final state occurs at most once per start position (and a selection picks at
// most one record per position), so a partial is bounded by the positions its workgroup sees.  A scan owns at most
// 2^32 positions in 2^20 tiles, dealt round-robin to the grid's waves, and the host never launches fewer than two
// workgroups: one sees at most 2^19 tiles (2^25 chunks of a selection) = 2^31 positions.
// 64 lanes adding to ONE LDS address serialise, and with one hot pattern that is every chunk.  So a chunk can be
// pre-aggregated in the wave: the first lane that holds a record names its state, a ballot finds the lanes that share
// it, that one lane adds their number, the lanes left over add their own 1.  Such a round costs about as much as 25
// serialised lanes, so it pays only where one state fills a good part of a chunk -- and loses
// 15 % on a dictionary.  The wave therefore PROBES: every COUNT_PROBE-th chunk it runs the round and keeps it on for
// the chunks that follow iff the leader's state held at least PFAC_COUNT_PEEL_MIN of the 64 lanes.
#ifndef PFAC_COUNT_PEEL
#define PFAC_COUNT_PEEL 1              // rounds of wave pre-aggregation per chunk (0: never; more than one lost everywhere)
#endif
#ifndef PFAC_COUNT_PEEL_MIN
#define PFAC_COUNT_PEEL_MIN 24         // lanes of the leader's state in a probed chunk that keep the round on (0: always on)
#endif
#ifndef PFAC_COUNT_PROBE
#define PFAC_COUNT_PROBE 16
#endif
constexpr unsigned COUNT_PROBE = PFAC_COUNT_PROBE;
constexpr int COUNT_THREADS = 256;             // a workgroup over a direct table: four waves ...
constexpr int COUNT_THREADS_MAX = 1024;        // ... over the cache: sixteen, ONE workgroup per CU
constexpr unsigned COUNT_DIRECT_MAX = 8192;    // states of a direct table, 4 B each: at most 32 KiB of LDS
constexpr unsigned COUNT_CACHE_SLOTS = 16384;  // slots of the cache, 8 B each: 128 KiB of the CU's 160
constexpr unsigned COUNT_BINS_MAX = COUNT_CACHE_SLOTS;     // (PFAC_COUNT_BINS: fewer of either)

__device__ __forceinline__ unsigned count_slot_of(unsigned state, unsigned bins) { return __umulhi(state * 0x9E3779B1u, bins); }

template <bool DIRECT>
__device__ __forceinline__ void count_add(unsigned *lds, unsigned bins, unsigned long long *counts, unsigned st, unsigned n) {
    if (DIRECT) {
        __hip_atomic_fetch_add(lds + st, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    unsigned *e = lds + 2 * count_slot_of(st, bins);
    const unsigned want = st + 1;
    unsigned tag = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (tag == 0) {
        const unsigned old = atomicCAS(e, 0u, want);
        tag = old ? old : want;
    }
    if (tag == want) __hip_atomic_fetch_add(e + 1, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_add(counts + st, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one chunk: `have` lanes hold a state below n_states (called by the whole wave; `phase` counts the wave's chunks,
// `peel` is what its last probe decided)
template <bool DIRECT>
__device__ __forceinline__ void count_chunk(unsigned *lds, unsigned bins, unsigned long long *counts, bool have, unsigned st, int lane,
                                            unsigned &phase, bool &peel) {
    bool todo = have;
    const bool probe = (phase++ % COUNT_PROBE) == 0;
    if (PFAC_COUNT_PEEL > 0 && (peel || probe)) {
#pragma unroll
        for (int r = 0; r < PFAC_COUNT_PEEL; r++) {
            const unsigned long long act = __ballot(todo);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const unsigned s0 = (unsigned)__builtin_amdgcn_readlane((int)st, leader);
            const bool mine = todo && st == s0;
            const unsigned n = (unsigned)__popcll(__ballot(mine));
            if (r == 0 && probe) peel = n >= (unsigned)PFAC_COUNT_PEEL_MIN;
            if (lane == leader) count_add<DIRECT>(lds, bins, counts, s0, n);
            todo = todo && !mine;
        }
    }
    if (todo) count_add<DIRECT>(lds, bins, counts, st, 1u);
}

// BYTES 0: the flat array `rec` of `cap` pfac_records (a selection) in n_items chunks of 64; else the heap behind the
// n_items tiles of tix.  No counter at or past n_states is ever written; res[0] += records counted.
template <int BYTES, bool DIRECT>
__global__ void __launch_bounds__(COUNT_THREADS_MAX)
pfac_count_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_items, unsigned long long cap, unsigned n_states,
                  unsigned bins, unsigned long long *counts, unsigned long long *res) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned *lds = reinterpret_cast<unsigned *>(smem);
    const unsigned words = DIRECT ? n_states : 2 * bins;
    for (unsigned i = threadIdx.x; i < words; i += blockDim.x) lds[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wstride = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    unsigned long long counted = 0;
    unsigned phase = 0;
    bool peel = false;
    for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n_items; t += wstride) {
        if (BYTES == 0) {
            const unsigned long long i = t * WAVE + lane, n = cap;      // (cap: the records of the array)
            unsigned st = 0;
            bool have = i < n;
            if (have) st = static_cast<const pfac_record *>(rec)[i].state;
            have = have && st < n_states;
            counted += have;
            count_chunk<DIRECT>(lds, bins, counts, have, st, lane, phase, peel);
        } else {
            const unsigned long long e = tix[t], lo = e & TIX_BASE_MASK;
            const unsigned cnt = (unsigned)(e >> TIX_CNT_SHIFT);
            for (unsigned i0 = 0; i0 < cnt; i0 += WAVE) {
                const unsigned i = i0 + (unsigned)lane;
                unsigned pos, st = 0;
                bool have = i < cnt && lo + i < cap;
                if (have) heap_record<(BYTES ? BYTES : 4)>(rec, lo + i, t, pos, st);
                have = have && st < n_states;
                counted += have;
                count_chunk<DIRECT>(lds, bins, counts, have, st, lane, phase, peel);
            }
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < (DIRECT ? n_states : bins); i += blockDim.x) {
        const unsigned c = DIRECT ? lds[i] : lds[2 * i + 1];
        const unsigned st = DIRECT ? i : lds[2 * i] - 1u;
        if (c) __hip_atomic_fetch_add(counts + st, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    counted = wave_sum64(counted);
    if (lane == 0 && counted) __hip_atomic_fetch_add(res, counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A caller's selection (d_sel) before it is counted: states below n_states, positions ascending.  bad[0] = 1 if not.
__global__ void pfac_sel_check_kernel(const pfac_record *sel, unsigned long long n, unsigned n_states, unsigned long long *bad) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    bool wrong = false;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const pfac_record r = sel[i];
        wrong = wrong || r.state >= n_states || (i + 1 < n && sel[i + 1].pos <= r.pos);
    }
    if (wrong) bad[0] = 1ull;
}

// Heap -> one sorted pfac_record array, three small kernels: records per group of 64 tiles, exclusive scan of the
// group sums (one block), copy.  Only consumers that want the flat sorted array pay for this.
constexpr int XGROUP = 64;
__global__ void pfac_tix_group_sum_kernel(const unsigned long long *tix, unsigned long long n_tiles, unsigned long long *gsum, unsigned n_groups) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned c = t < n_tiles ? (unsigned)(tix[t] >> TIX_CNT_SHIFT) : 0u;
    const unsigned long long sum = wave_sum64(c);
    if (lane == 0) gsum[g] = sum;
}
__global__ void pfac_scan_groups_kernel(unsigned long long *gsum, unsigned n_groups) {      // ONE block of 1024 threads
    __shared__ unsigned long long part[1024];
    const unsigned per = (n_groups + 1023u) / 1024u;
    const unsigned lo = threadIdx.x * per, hi = lo + per < n_groups ? lo + per : n_groups;
    unsigned long long sum = 0;
    for (unsigned i = lo; i < hi; i++) sum += gsum[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long acc = 0;
        for (int i = 0; i < 1024; i++) { const unsigned long long v = part[i]; part[i] = acc; acc += v; }
    }
    __syncthreads();
    unsigned long long acc = part[threadIdx.x];
    for (unsigned i = lo; i < hi; i++) { const unsigned long long v = gsum[i]; gsum[i] = acc; acc += v; }
    if (hi == n_groups && lo < hi) gsum[n_groups] = acc;       // (the thread that owns the last group: the grand total)
}
// records [first, first + n) of the sorted sequence -> out[0, n)
template <int BYTES>
__global__ void pfac_expand_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles,
                                   const unsigned long long *gpre, unsigned n_groups, unsigned long long cap,
                                   unsigned long long first, unsigned long long n, pfac_record *out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    const unsigned long long off = gpre[g] + (wave_incl_scan(c) - c);     // sorted index of the tile's first record (< 2^32 per group)
    const unsigned long long end = first + n;
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE), toff = __shfl(off, j, WAVE);
        if (toff >= end || toff + tc <= first) continue;
        for (unsigned i = (unsigned)lane; i < tc; i += WAVE) {
            const unsigned long long k = toff + i;
            if (k < first || k >= end || tlo + i >= cap) continue;
            pfac_record o;
            heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, o.pos, o.state);
            out[k - first] = o;
        }
    }
}

// ---------------------------------------------------------------------------
// Documents (pfac_records_segment): the records of a scan over a concatenation of documents, cut at the document ends.
// A record (pos, state) belongs to document d = the last one with off[d] <= pos, and is kept iff
// pos + len[state] <= off[d + 1].  Same three-kernel shape as the expand path: kept records per tile and per group of
// 64 tiles (the offsets are checked in the same pass), pfac_scan_groups_kernel over the group sums, then the write.
// A tile's documents are found by binary search in the offsets: [ds, de) start in it (the last tile also takes the
// documents that start at n_owned), and ds - 1 runs into it; a record searches only that small range.

// first d in [0, n) with off[d] >= x (n if none)
__device__ __forceinline__ unsigned long long doc_lower_bound(const unsigned long long *off, unsigned long long n, unsigned long long x) {
    unsigned long long lo = 0, hi = n;
    while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (off[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the last d in [lo, hi] with off[d] <= pos (lo when none: off[lo] <= pos holds for valid offsets)
__device__ __forceinline__ unsigned long long doc_of(const unsigned long long *off, unsigned long long lo, unsigned long long hi, unsigned long long pos) {
    while (lo < hi) {
        const unsigned long long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= pos) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// documents [*ds, *de) start in tile t; a record of the tile lies in one of [*dlo, *dhi] (clamped to [0, n_docs - 1],
// so that off[d + 1] stays in bounds while the offsets are still unchecked)
__device__ __forceinline__ void tile_docs(const unsigned long long *off, unsigned long long n_docs, unsigned long long t,
                                          unsigned long long n_tiles, unsigned long long &ds, unsigned long long &de,
                                          unsigned long long &dlo, unsigned long long &dhi) {
    ds = doc_lower_bound(off, n_docs + 1, t * WTILE);
    de = t + 1 == n_tiles ? n_docs + 1 : doc_lower_bound(off, n_docs + 1, (t + 1) * WTILE);
    const unsigned long long top = n_docs - 1;
    dlo = ds ? ds - 1 : 0;
    dhi = de ? de - 1 : 0;
    if (dlo > top) dlo = top;
    if (dhi > top) dhi = top;
    if (dhi < dlo) dhi = dlo;
}

// The documents a record of one tile can lie in, [dlo, dhi]: when off[dlo .. dhi + 1] fit one per lane (a tile holds
// fewer than 63 document starts -- every document of 64 bytes or more), lane k holds off[dlo + k] and a record finds its
// document by a binary search over the lanes (shuffles, no memory); else by a binary search in the offsets themselves.
struct DocWin {
    unsigned long long dlo, dhi, woff;
    unsigned n, top;                                           // candidates (dhi - dlo + 1), highest power of two below n
    bool win;
};
__device__ __forceinline__ DocWin doc_window(const unsigned long long *off, unsigned long long dlo, unsigned long long dhi, int lane) {
    DocWin w;
    w.dlo = dlo;
    w.dhi = dhi;
    w.win = dhi - dlo + 2 <= (unsigned long long)WAVE;
    w.n = w.win ? (unsigned)(dhi - dlo + 1) : 0u;
    w.top = w.n > 1 ? 1u << (31 - __clz(w.n - 1)) : 0u;
    w.woff = w.win && (unsigned)lane <= w.n ? off[dlo + lane] : ~0ull;
    return w;
}
// record at pos -> its document d, off[d], off[d + 1] (every lane takes part: the shuffles)
__device__ __forceinline__ void doc_lookup(const DocWin &w, const unsigned long long *off, bool have, unsigned pos,
                                           unsigned long long &d, unsigned long long &base, unsigned long long &end) {
    if (w.win) {
        unsigned k = 0;
        for (unsigned step = w.top; step; step >>= 1) {
            const unsigned cand = k + step;
            const unsigned long long v = __shfl(w.woff, cand < w.n ? cand : 0u, WAVE);
            if (cand < w.n && v <= pos) k = cand;
        }
        d = w.dlo + k;
        base = __shfl(w.woff, k, WAVE);
        end = __shfl(w.woff, k + 1, WAVE);
    } else {
        d = have ? doc_of(off, w.dlo, w.dhi, pos) : w.dlo;
        base = have ? off[d] : 0ull;
        end = have ? off[d + 1] : 0ull;
    }
}
// pattern length of final state st: from a register of lane st when the table has at most 64 final states
__device__ __forceinline__ int final_len(const short *flen, int freg, bool fsmall, bool have, unsigned st) {
    if (fsmall) return __shfl(freg, (int)st, WAVE);
    return have ? (int)flen[st] : 0;
}
// The offsets' rules (off[0] == 0, no decrease, off[n_docs] == n_owned), one thread per document, grid-stride: a flag,
// and the host writes nothing behind it.  Called by the first kernel of every document-aware pass, and by
// pfac_offsets_check_kernel where no such kernel runs.  The thread's index in the grid and the grid's size come from the
// kernel (GRID_THREAD, GRID_THREADS, #undef'd behind the last of the three): the workgroup's size folds to a load of
// the kernel's arguments only in a kernel's own body; read in here the three kernels compile to other code than the
// parent's (DESIGN.md section 19 has the figures).
#define GRID_THREAD ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x)
#define GRID_THREADS ((unsigned long long)gridDim.x * blockDim.x)
__device__ __forceinline__ void offsets_rule(unsigned long long gtid, unsigned long long gstride, const unsigned long long *off,
                                             unsigned long long n_docs, unsigned long long n_owned, unsigned long long *bad) {
    for (unsigned long long d = gtid; d < n_docs; d += gstride)
        if (off[d] > off[d + 1]) *bad = 1ull;
    if (gtid == 0 && (off[0] != 0ull || off[n_docs] != n_owned)) *bad = 1ull;
}
__global__ void pfac_offsets_check_kernel(const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                                          unsigned long long *bad) {
    offsets_rule(GRID_THREAD, GRID_THREADS, off, n_docs, n_owned, bad);
}

template <int BYTES>
__global__ void pfac_seg_count_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                      const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                                      const short *flen, unsigned num_final, unsigned *tcnt, unsigned long long *gsum,
                                      unsigned n_groups, unsigned long long *bad) {
    offsets_rule(GRID_THREAD, GRID_THREADS, off, n_docs, n_owned, bad);
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (c) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    unsigned mine = 0;                                          // kept records of tile t
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        const DocWin w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
        unsigned kept = 0;
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            const int len = final_len(flen, freg, fsmall, have, st);
            unsigned long long d, base, end;
            doc_lookup(w, off, have, pos, d, base, end);
            const bool keep = have && len > 0 && (unsigned long long)pos + (unsigned)len <= end;
            kept += (unsigned)__popcll(__ballot(keep));
        }
        if (lane == j) mine = kept;
    }
    if (t < n_tiles) tcnt[t] = mine;
    const unsigned long long sum = wave_sum64(mine);
    if (lane == 0) gsum[g] = sum;
}

// kept records -> out[k] = {pos - off[d], state} at their sorted index k; doc_first[d] for every document that starts
// in the tile: the index of the first kept record of a document >= d (a document without kept records gets the index
// of the next one's, the documents behind the last kept record the index past the tile's)
template <int BYTES>
__global__ void pfac_seg_write_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                      const unsigned long long *off, unsigned long long n_docs, const short *flen, unsigned num_final,
                                      const unsigned *tcnt, const unsigned long long *gpre, unsigned n_groups,
                                      pfac_record *out, unsigned long long *doc_first) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    const unsigned kc = t < n_tiles ? tcnt[t] : 0u;
    const unsigned long long off0 = gpre[g] + (wave_incl_scan(kc) - kc);   // sorted index of the tile's first kept record
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (t < n_tiles) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    for (int j = 0; j < XGROUP; j++) {
        if ((unsigned long long)g * XGROUP + j >= n_tiles) break;
        const unsigned tc = __shfl(c, j, WAVE);
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        const unsigned long long tde = __shfl(de, j, WAVE);
        unsigned long long k = __shfl(off0, j, WAVE);           // next output index (wave-uniform)
        unsigned long long nxt = __shfl(ds, j, WAVE);           // first document of the tile whose doc_first is not written yet
        const unsigned kt = __shfl(kc, j, WAVE);
        if (kt) {                                               // (a tile without kept records only places its documents)
            const DocWin w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
            for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
                const unsigned i = c0 + (unsigned)lane;
                const bool have = i < tc && tlo + i < cap;
                unsigned pos = 0, st = 0;
                if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
                const int len = final_len(flen, freg, fsmall, have, st);
                unsigned long long d, base, end;
                doc_lookup(w, off, have, pos, d, base, end);
                const bool keep = have && len > 0 && (unsigned long long)pos + (unsigned)len <= end;
                const unsigned long long b = __ballot(keep);
                if (b == 0) continue;
                const unsigned long long below = b & ((1ull << lane) - 1ull);    // kept lanes in front of this one
                const unsigned long long dprev = __shfl(d, below ? 63 - __clzll(below) : lane, WAVE);
                if (keep) {
                    const unsigned long long kk = k + (unsigned)__popcll(below);
                    pfac_record o;
                    o.pos = pos - (unsigned)base;
                    o.state = st;
                    out[kk] = o;
                    for (unsigned long long dd = below ? dprev + 1 : nxt; dd <= d; dd++) doc_first[dd] = kk;
                }
                nxt = __shfl(d, 63 - __clzll(b), WAVE) + 1;
                k += (unsigned)__popcll(b);
            }
        }
        for (unsigned long long dd = nxt + lane; dd < tde; dd += WAVE) doc_first[dd] = k;
    }
}

// ---------------------------------------------------------------------------
// Per-document reductions straight from the heap: pattern groups (pfac_documents_group_masks, mask[d] = the OR of
// gmask[state]) and scores (pfac_documents_scores, {score, count}[d] = the sum of {weight[state], 1}), both over the
// records the segment pass would keep for document d -- the walk of pfac_seg_count_kernel (record, length, document, keep
// rule; the offsets' rules in the same pass) with one value per DOCUMENT behind it instead of a count per tile, and no
// global atomic per record.  ONE kernel, pfac_doc_reduce_kernel, templated on the reduction (GroupOr, ScoreAdd below):
// the value types (a lane's inside a chunk, a run's across chunks), what a kept record brings, which lanes contribute,
// the combines, the store and the atomic.
// One wave per group of 64 tiles.  A tile's records come in position order, so the documents of the contributing lanes
// ascend: every lane takes the document of the nearest contributing lane at or below it (the first one's in front of
// it) with the neutral value where it contributes nothing, and a segmented inclusive scan keyed on the document (six
// shuffle steps, doc_reduce_chunk) leaves each run's value in its last lane.  The chunk's last run stays open in two
// wave-uniform registers (cd, cm) across chunks and tiles; a run is flushed ONCE, when the document changes or the
// wave's tiles end.
// Exactly once, which a sum needs and an OR did not: the open run (cd, cm) enters a chunk only through the lanes whose
// key equals cd.  Keys ascend and cd is at most the first key, so those lanes are a prefix of the chunk, and cm goes
// into every one of them -- they hold INCLUSIVE prefixes of the run, of which only the last lane's is ever used: it is
// flushed where the next lane's key differs, or it leaves through lane 63 as the new (cd, cm).  Where no key equals cd
// the run is closed and lane 0 flushes it as it stands.  Either way cm is consumed by one flush or one carry, never both.
// Who contributes: GroupOr the lanes whose kept record has a mask (a mask of 0 changes nothing, the document keeps the
// memset's 0); ScoreAdd every lane that KEEPS its record -- a weight of 0 still counts, and weights that cancel still
// leave a count to write.
// Who writes out[d]: the wave's tiles cover the bytes [B0, B1) and every record of them starts there.  A document with
// B0 <= off[d] and off[d + 1] <= B1 gets all its records from this wave, which flushes it once: a plain store of the
// whole value (8 or 16 bytes) over the zero that the host's memset left.  The others -- at most the one that runs in from
// below B0 and the one that runs out past B1 -- may be flushed by several waves and are combined with agent-scope atomics
// whose result nobody reads (one OR; two 64-bit adds, of which nobody needs the pair to be seen together before the
// kernel ends); no wave ever stores plainly to them, so store and atomic never meet on one word.  The interior documents
// are [a, e - 1) with a = the first d with off[d] >= B0 and e = the first index with off[e] > B1 (the last wave has no
// B1): two binary searches per wave.  Documents without a contributing record are never written -- the memset is their 0.
// With offsets that break the rules the documents stay clamped to [0, n_docs) (tile_docs), the result is garbage in
// bounds, and the host discards it behind the flag.
struct GroupOr {
    using Tab = unsigned long long;                             // per final state: its group set
    using Lane = unsigned long long;                            // what a lane carries through a chunk's scan, ...
    using Val = unsigned long long;                             // ... and what a run is worth once it meets the open run
    using Out = unsigned long long;
    static constexpr int RES_WORDS = 1;                         // res[0]: the OR of all masks; res[RES_WORDS]: bad offsets
    static __device__ __forceinline__ Lane lane_none() { return 0ull; }
    static __device__ __forceinline__ Lane of(Tab t) { return t; }
    static __device__ __forceinline__ bool contributes(bool, Lane v) { return v != 0ull; }
    static __device__ __forceinline__ void lane_add(Lane &a, Lane b) { a |= b; }
    static __device__ __forceinline__ Lane lane_shfl_up(Lane v, int s) { return __shfl_up(v, s, WAVE); }
    static __device__ __forceinline__ Val widen(Lane v) { return v; }
    static __device__ __forceinline__ Val none() { return 0ull; }
    static __device__ __forceinline__ bool empty(Val v) { return v == 0ull; }
    static __device__ __forceinline__ void add(Val &a, Val b) { a |= b; }
    static __device__ __forceinline__ Val shfl(Val v, int l) { return __shfl(v, l, WAVE); }
    static __device__ __forceinline__ void store(Out *out, unsigned d, Val v) { out[d] = v; }
    static __device__ __forceinline__ void atomic(Out *out, unsigned d, Val v) {
        (void)__hip_atomic_fetch_or(out + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void total(unsigned long long *res, Val any, int lane) {
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) any |= __shfl_xor(any, s, WAVE);
        if (lane == 0 && any) (void)__hip_atomic_fetch_or(res, any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct ScoreAdd {
    using Tab = int;                                            // per final state: its weight
    // Inside a chunk a run holds at most 64 records: its count fits 8 bits and its score, below 2^37 in size, the 56
    // above them, so a lane carries score * 256 + count in ONE word and the scan shuffles what the mask pass shuffles.
    using Lane = unsigned long long;
    struct Val { unsigned long long s, c; };                    // the score (two's complement: it wraps) and the count
    using Out = pfac_doc_score;
    static constexpr int RES_WORDS = 2;                         // res[0], res[1]: the totals; res[RES_WORDS]: the pass's flag
    static __device__ __forceinline__ Lane lane_none() { return 0ull; }
    static __device__ __forceinline__ Lane of(Tab t) { return ((unsigned long long)(long long)t << 8) + 1ull; }
    static __device__ __forceinline__ bool contributes(bool keep, Lane) { return keep; }
    static __device__ __forceinline__ void lane_add(Lane &a, Lane b) { a += b; }
    static __device__ __forceinline__ Lane lane_shfl_up(Lane v, int s) { return __shfl_up(v, s, WAVE); }
    static __device__ __forceinline__ Val widen(Lane v) {
        const unsigned long long c = v & 255ull;
        return Val{(unsigned long long)((long long)(v - c) >> 8), c};
    }
    static __device__ __forceinline__ Val none() { return Val{0ull, 0ull}; }
    static __device__ __forceinline__ bool empty(Val) { return false; }      // (a run holds a kept record: count >= 1)
    static __device__ __forceinline__ void add(Val &a, Val b) { a.s += b.s; a.c += b.c; }
    static __device__ __forceinline__ Val shfl(Val v, int l) { return Val{__shfl(v.s, l, WAVE), __shfl(v.c, l, WAVE)}; }
    static __device__ __forceinline__ void store(Out *out, unsigned d, Val v) {       // one dwordx4
        reinterpret_cast<ulonglong2 *>(out)[d] = make_ulonglong2(v.s, v.c);
    }
    static __device__ __forceinline__ void atomic(Out *out, unsigned d, Val v) {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(out + d);
        (void)__hip_atomic_fetch_add(w, v.s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(w + 1, v.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    static __device__ __forceinline__ void total(unsigned long long *res, Val any, int lane) {
        const unsigned long long s = wave_sum64(any.s), c = wave_sum64(any.c);
        if (lane == 0 && c) {
            (void)__hip_atomic_fetch_add(res, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(res + 1, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

// One chunk of 64 lanes of a per-document reduction: lane values lm (R::lane_none() where the lane does not
// contribute), the contributing lanes b (not empty) and their documents d, ascending; (cvalid, cd, cm) is the open run,
// flush(d, value) closes one.  Every lane of the wave takes part.
template <class R, class Flush>
__device__ __forceinline__ void doc_reduce_chunk(int lane, unsigned long long b, unsigned long long d, typename R::Lane lm, bool &cvalid,
                                                 unsigned &cd, typename R::Val &cm, Flush flush) {
    const unsigned long long below = b & ((2ull << lane) - 1ull);        // contributing lanes up to this one
    unsigned dk = (unsigned)__shfl((unsigned)d, below ? 63 - __clzll(below) : __ffsll((long long)b) - 1, WAVE);
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        const unsigned du = (unsigned)__shfl_up(dk, s, WAVE);
        const typename R::Lane mu = R::lane_shfl_up(lm, s);
        if (lane >= s && du == dk) R::lane_add(lm, mu);
    }
    typename R::Val m = R::widen(lm);
    if (cvalid) {
        if (__ballot(dk == cd) != 0ull) {
            if (dk == cd) R::add(m, cm);                        // the open run goes on (it starts at lane 0)
        } else if (lane == 0) {
            flush(cd, cm);
        }
    }
    const unsigned dn = (unsigned)__shfl_down(dk, 1, WAVE);
    if (lane != WAVE - 1 && dn != dk) flush(dk, m);
    cd = (unsigned)__shfl(dk, WAVE - 1, WAVE);
    cm = R::shfl(m, WAVE - 1);
    cvalid = true;
}

template <int BYTES, class R>
__global__ void __launch_bounds__(256)
pfac_doc_reduce_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                       const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                       const short *flen, const typename R::Tab *tab, unsigned num_final, typename R::Out *out,
                       unsigned n_groups, unsigned long long *res) {         // res: R::RES_WORDS totals, then bad offsets
    using Val = typename R::Val;
    offsets_rule(GRID_THREAD, GRID_THREADS, off, n_docs, n_owned, res + R::RES_WORDS);
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    const typename R::Tab greg = fsmall && (unsigned)lane < num_final ? tab[lane] : typename R::Tab(0);
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    if (__ballot(c != 0u) == 0ull) return;                      // a range without records writes nothing
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (c) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    // the documents this wave alone writes: [ia, ie)
    const bool last = ((unsigned long long)g + 1) * XGROUP >= n_tiles;
    const unsigned long long ia = doc_lower_bound(off, n_docs + 1, (unsigned long long)g * XGROUP * WTILE);
    const unsigned long long ib = last ? n_docs + 1 : doc_lower_bound(off, n_docs + 1, ((unsigned long long)g + 1) * XGROUP * WTILE + 1ull);
    const unsigned long long ie = ib ? ib - 1 : 0ull;
    auto flush = [&](unsigned d, Val m) {
        if (R::empty(m)) return;
        if (d >= ia && d < ie) R::store(out, d, m);
        else R::atomic(out, d, m);
    };
    bool cvalid = false;                                        // the open run (wave-uniform)
    unsigned cd = 0;
    Val cm = R::none(), any = R::none();
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        const DocWin w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            const int len = final_len(flen, freg, fsmall, have, st);
            const typename R::Tab gm = fsmall ? __shfl(greg, (int)st, WAVE) : (have ? tab[st] : typename R::Tab(0));
            unsigned long long d, base, end;
            doc_lookup(w, off, have, pos, d, base, end);
            const bool keep = have && len > 0 && (unsigned long long)pos + (unsigned)len <= end;
            const typename R::Lane m = keep ? R::of(gm) : R::lane_none();
            const unsigned long long b = __ballot(R::contributes(keep, m));
            if (b == 0ull) continue;
            R::add(any, R::widen(m));
            doc_reduce_chunk<R>(lane, b, d, m, cvalid, cd, cm, flush);
        }
    }
    if (cvalid && lane == 0) flush(cd, cm);
    R::total(res, any, lane);
}

// Scores of a record array that is already cut per document (pfac_selection_document_scores): document d owns
// sel[first[d] .. first[d + 1]), n = first[n_docs] records in all.  Pick-driven: a wave owns SS_RANGE consecutive picks,
// a lane takes one record; its document is the last d with first[d] <= i, searched between the documents of the
// chunk's first and last pick (two wave-uniform searches; none per lane where those two agree).  Every pick
// contributes; the same segmented add (doc_reduce_chunk<ScoreAdd>) and the same rule for the store: the documents whose
// picks lie inside the wave's range, [ia, ie) by the two searches of the heap kernel, are stored plainly, the two that
// may straddle its ends are added atomically.  Checked in the same pass, into res[2]: first[0] == 0, no decrease,
// first[n_docs] == n, every state below num_final (a state past the table reads no weight).  Behind a failed check the
// result is garbage in bounds -- documents stay in [0, n_docs) -- and the host discards it.
constexpr unsigned SS_RANGE = 4 * WAVE;
__global__ void __launch_bounds__(256)
pfac_sel_scores_kernel(const pfac_record *sel, unsigned long long n, const unsigned long long *first, unsigned long long n_docs,
                       const int *wtab, unsigned num_final, pfac_doc_score *out, unsigned long long *res) {
    using R = ScoreAdd;
    bool bad = false;
    for (unsigned long long d = GRID_THREAD; d < n_docs; d += GRID_THREADS) bad = bad || first[d] > first[d + 1];
    if (GRID_THREAD == 0) bad = bad || first[0] != 0ull || first[n_docs] != n;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long p0 = ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SS_RANGE;
    if (p0 < n && n_docs) {                                     // (wave-uniform)
        const unsigned long long p1 = min(p0 + SS_RANGE, n);
        const bool fsmall = num_final <= (unsigned)WAVE;
        const int wreg = fsmall && (unsigned)lane < num_final ? wtab[lane] : 0;
        const unsigned long long ia = doc_lower_bound(first, n_docs + 1, p0);
        const unsigned long long ib = p1 >= n ? n_docs + 1 : doc_lower_bound(first, n_docs + 1, p1 + 1ull);
        const unsigned long long ie = ib ? ib - 1 : 0ull;
        auto flush = [&](unsigned d, R::Val m) {
            if (d >= ia && d < ie) R::store(out, d, m);
            else R::atomic(out, d, m);
        };
        bool cvalid = false;
        unsigned cd = 0;
        R::Val cm = R::none(), any = R::none();
        unsigned long long dlo = 0;
        for (unsigned long long c0 = p0; c0 < p1; c0 += WAVE) {
            const unsigned long long i = c0 + (unsigned)lane;
            const bool have = i < p1;
            dlo = doc_of(first, dlo, n_docs - 1, c0);
            const unsigned long long dhi = doc_of(first, dlo, n_docs - 1, min(c0 + (WAVE - 1), p1 - 1));
            const unsigned st = have ? sel[i].state : 0u;
            const bool known = st < num_final;
            bad = bad || !known;
            const int wt = fsmall ? __shfl(wreg, known ? (int)st : 0, WAVE) : (have && known ? wtab[st] : 0);
            const unsigned long long d = have ? doc_of(first, dlo, dhi, i) : dlo;
            const R::Lane m = have ? R::of(known ? wt : 0) : R::lane_none();
            R::add(any, R::widen(m));
            doc_reduce_chunk<R>(lane, __ballot(have), d, m, cvalid, cd, cm, flush);
        }
        if (cvalid && lane == 0) flush(cd, cm);
        R::total(res, any, lane);
    }
    if (bad) res[R::RES_WORDS] = 1ull;
}

// ---------------------------------------------------------------------------
// Whole-word filter (pfac_records_filter_words): drops, IN PLACE, the records that split a word.  With W the 256-bit
// set of word bytes, cut(i) = W(in[i-1]) && W(in[i]) (in[-1] = prev, in[n_avail] = next, -1 = no byte; never at a
// document offset); a record (pos, state) of length L goes when its tested edge(s) cut: cut(pos), cut(pos + L).
// One wave per tile at a time, a group of 64 tiles per wave as in the expand and segment kernels.  Per chunk of 64
// records: the record, its length, up to four byte gathers, a ballot, and the kept words stored to
// FIRST + kept so far + rank.  Why in place is safe: the stores of chunk k depend on the ballot over ALL lanes' loads
// of chunk k, so those loads have completed; they land in [FIRST, FIRST + 64 (k + 1)), and chunk k + 1 loads from
// FIRST + 64 (k + 1) on -- a later chunk is never clobbered, whichever way the two are scheduled.  Stores are as wide
// as a record (a 2-byte store for 16-bit words: the neighbouring tile's run may share the dword, and another wave
// owns it).  The tile index keeps FIRST and gets the new COUNT; the kept total goes through one atomicAdd per wave.
template <int BYTES>
__device__ __forceinline__ void heap_put(void *rec, unsigned long long i, unsigned pos, unsigned state) {
    if (BYTES == 2) {
        static_cast<unsigned short *>(rec)[i] = (unsigned short)((pos & 0xFFFu) | state << 12);
    } else if (BYTES == 4) {
        static_cast<unsigned *>(rec)[i] = (pos & 0xFFFu) | state << 12;
    } else {
        pfac_record r;
        r.pos = pos;
        r.state = state;
        static_cast<pfac_record *>(rec)[i] = r;
    }
}
struct WordSet {
    unsigned long long w[4];
};
// W(b) for b in -1..255 (-1: no byte there)
__device__ __forceinline__ bool word_byte(const WordSet &ws, int b) {
    if (b < 0) return false;
    const unsigned long long lo = (b & 64) ? ws.w[1] : ws.w[0], hi = (b & 64) ? ws.w[3] : ws.w[2];
    return (((b & 128) ? hi : lo) >> (b & 63)) & 1ull;
}
template <int BYTES, bool DOCS>
__global__ void pfac_filter_words_kernel(void *rec, unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                         const unsigned char *in, unsigned long long n_avail, const short *flen,
                                         unsigned num_final, WordSet ws, unsigned edges, int prev_byte, int next_byte,
                                         const unsigned long long *off, unsigned long long n_docs,
                                         const unsigned long long *bad, unsigned long long *total) {
    if (DOCS && *bad) return;                                   // offsets that break the rules: nothing is touched
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (DOCS && c) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    unsigned mine = c;                                          // records tile t keeps
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        DocWin w;
        if (DOCS) w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
        unsigned kept = 0;
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            const int len = final_len(flen, freg, fsmall, have, st);
            const unsigned long long end = (unsigned long long)pos + (unsigned)(len > 0 ? len : 0);
            const bool ok = have && len > 0;                    // (a state without a length never occurs in a record)
            bool lcut = false, rcut = false;
            if (ok && (edges & PFAC_WORD_LEFT)) {
                const int a = pos ? (int)in[pos - 1] : prev_byte;
                lcut = word_byte(ws, a) && pos < n_avail && word_byte(ws, (int)in[pos]);
            }
            if (ok && (edges & PFAC_WORD_RIGHT) && end <= n_avail) {
                const int b = end < n_avail ? (int)in[end] : next_byte;
                rcut = word_byte(ws, b) && word_byte(ws, (int)in[end - 1]);
            }
            if (DOCS) {                                         // no cut at a document offset
                unsigned long long d, dbase, dend;
                doc_lookup(w, off, have, pos, d, dbase, dend);
                if (dbase == pos) lcut = false;
                if (rcut) {
                    if (end == dend) rcut = false;
                    else if (end > dend) {                      // runs across its document's end: any later offset?
                        const unsigned long long k = doc_lower_bound(off, n_docs + 1, end);
                        if (k <= n_docs && off[k] == end) rcut = false;
                    }
                }
            }
            const bool keep = have && !lcut && !rcut;
            const unsigned long long b = __ballot(keep);
            const unsigned to = kept + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
            if (keep && to != i) heap_put<BYTES>(rec, tlo + to, pos, st);
            kept += (unsigned)__popcll(b);
        }
        if (lane == j) mine = kept;
    }
    if (t < n_tiles && mine != c) tix[t] = lo | (unsigned long long)mine << TIX_CNT_SHIFT;
    const unsigned long long sum = wave_sum64(mine);
    if (lane == 0 && sum) atomicAdd(total, sum);
}

// ---------------------------------------------------------------------------
// Span filter (pfac_records_filter_spans): the positional sibling of the whole-word filter -- drops, IN PLACE, the
// records that start or end where their state's span (pfac_state_span) does not admit them.  With d the record's
// document [base, E) (DOCS; else [0, n_avail)), rel = pos - base, C = E - 1 if the document ends in the delimiter, else
// E, and tail = C - (pos + L), 0 where the match covers the delimiter, infinite where it runs across E:
//   kept iff min_start <= rel <= max_start && (max_tail == PFAC_SPAN_ANY || tail <= max_tail).
// LINE judges every state as {0, 0, 0} and loads no span.  The input is read for in[E - 1] alone, by the records whose
// tail is judged and end inside their document, and only with a delimiter (E <= n_avail: the read stays in the buffer).
// The grid and the walk are the whole-word filter's: one wave per tile at a time, 64 tiles per wave; per chunk of 64
// records the record, its length, its span -- ONE 16-byte gather, or three shuffles from lane `state` when the table
// has at most 64 final states -- its document (doc_window / doc_lookup), a ballot, heap_put at FIRST + kept + rank.
// In place is safe for the same reason: the stores of chunk k depend on the ballot over ALL lanes' loads of chunk k, so
// those loads have completed; they land in [FIRST, FIRST + 64 (k + 1)), at or below the chunk's own slots, and chunk
// k + 1 loads from FIRST + 64 (k + 1) on.  Stores are record-wide (2 bytes for a 16-bit word: the dword may be shared
// with the neighbouring tile's run, which another wave owns).  One atomicAdd per wave carries the kept total.
template <int BYTES, bool DOCS, bool LINE>
__global__ void pfac_filter_spans_kernel(void *rec, unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                         const unsigned char *in, unsigned long long n_avail, const short *flen,
                                         const uint4 *spans, unsigned num_final, int delimiter,
                                         const unsigned long long *off, unsigned long long n_docs,
                                         const unsigned long long *bad, unsigned long long *total) {
    if (DOCS && *bad) return;                                   // offsets that break the rules: nothing is touched
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    uint4 sreg = make_uint4(0u, LINE ? 0u : PFAC_SPAN_ANY, LINE ? 0u : PFAC_SPAN_ANY, 0u);
    if (!LINE && fsmall && (unsigned)lane < num_final) sreg = spans[lane];
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (DOCS && c) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    unsigned mine = c;                                          // records tile t keeps
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        DocWin w;
        if (DOCS) w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
        unsigned kept = 0;
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            const int len = final_len(flen, freg, fsmall, have, st);
            unsigned smin = 0, smax = 0, stail = 0;             // (LINE: {0, 0, 0})
            if (!LINE) {
                if (fsmall) {
                    smin = __shfl(sreg.x, (int)st, WAVE);
                    smax = __shfl(sreg.y, (int)st, WAVE);
                    stail = __shfl(sreg.z, (int)st, WAVE);
                } else if (have) {
                    const uint4 sp = spans[st];
                    smin = sp.x; smax = sp.y; stail = sp.z;
                }
            }
            unsigned long long dbase = 0, dend = n_avail;       // no documents: the one document [0, n_avail)
            if (DOCS) {
                unsigned long long d;
                doc_lookup(w, off, have, pos, d, dbase, dend);
            }
            const unsigned long long rel = (unsigned long long)pos - dbase;
            bool keep = have && rel >= smin && rel <= smax;
            if (keep && stail != PFAC_SPAN_ANY) {
                const unsigned long long pe = (unsigned long long)pos + (unsigned)(len > 0 ? len : 0);
                if (pe > dend) keep = false;                    // runs across its document's end: the tail is infinite
                else {
                    unsigned long long cend = dend;             // a line keeps its delimiter: `$` sits in front of it
                    if (delimiter >= 0 && dend > dbase && (int)in[dend - 1] == delimiter) cend = dend - 1;
                    keep = pe >= cend || cend - pe <= stail;    // (pe > cend: the match covers the delimiter, tail 0)
                }
            }
            const unsigned long long b = __ballot(keep);
            const unsigned to = kept + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
            if (keep && to != i) heap_put<BYTES>(rec, tlo + to, pos, st);
            kept += (unsigned)__popcll(b);
        }
        if (lane == j) mine = kept;
    }
    if (t < n_tiles && mine != c) tix[t] = lo | (unsigned long long)mine << TIX_CNT_SHIFT;
    const unsigned long long sum = wave_sum64(mine);
    if (lane == 0 && sum) atomicAdd(total, sum);
}

// ---------------------------------------------------------------------------
// Leftmost-longest non-overlapping selection (pfac_records_leftmost_longest).  The greedy -- from cursor c take the
// first position p >= c that has a record, its longest record, c = p + len -- is sequential, but with
// M = max_pat_len the cursor that reaches tile t lies in [4096t, 4096t + M]: every earlier pick started before the
// tile and is at most M long.  So tile t is a function F_t: [0, M] -> [0, M] from its entry offset to the exit offset
// into tile t + 1 (0 when the cursor ends before that tile starts; the last tile's exit is relative to n_owned), and
// composition is associative:
//   pfac_ll_tiles_kernel<., false>  one workgroup per group of 64 tiles, one tile per wave at a time in LDS;
//                                   G_g = F_{64g+63} o ... o F_{64g} as uint16[M + 1]
//   pfac_ll_compose_kernel          the G_g of 64 groups -> one function (two levels, no long dependent chain)
//   pfac_ll_walk_kernel             evaluates them from `entry`: every block's, then every group's entry offset
//   pfac_ll_tiles_kernel<., true>   the tile functions again; each tile's entry from its group's; the chain from that
//                                   entry marked in a per-tile bitmap of positions; selected records per tile, group
//   pfac_scan_groups_kernel, then pfac_ll_write_kernel: a selected record's index is its tile's prefix + ballot rank.
// Inside a tile: candidates k = the last record at each position (the longest), in position order; next[k] = the first
// candidate at or after pos[k] + len[k] (K: none, the chain leaves the tile).  Fewer than len[k] candidates lie in
// between, so a binary search over [k + 1, k + len] finds it.  The end of k's chain, exitE[k], comes from chunks of 64
// candidates in DESCENDING order: pointer jumping inside the chunk with lane shuffles (6 rounds), then the exitE of the
// first node past the chunk, already final, from LDS.  O(K log M) per tile whatever the input; chains that never meet
// (`aa` on a run of `a`) cost nothing extra.

constexpr int LL_WAVES = 4;                                     // waves per workgroup of the tiles kernel: one tile each
constexpr int LL_WAVE_LDS = WTILE * 2 * 3;                      // cpos, nxt, ends (u16 per candidate); the bitmap reuses ends
constexpr int LL_CHUNK_BYTES = 32768;                           // functions staged in LDS at a time by compose / walk

__host__ __device__ constexpr unsigned ll_fun_stride(unsigned m1) { return (m1 + 7u) & ~7u; }   // u16 per function (16-B rows)
static size_t ll_tiles_lds(unsigned m1) {
    return (size_t)LL_WAVES * LL_WAVE_LDS + (size_t)(LL_WAVES + 1) * ll_fun_stride(m1) * 2 + (2 * LL_WAVES + 2) * 8;
}

// first k in [lo, hi) with cpos[k] >= x (hi if none)
__device__ __forceinline__ unsigned ll_lower_bound(const unsigned short *cpos, unsigned lo, unsigned hi, unsigned x) {
    while (lo < hi) {
        const unsigned mid = (lo + hi) >> 1;
        if (cpos[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The candidate rule of the per-document selection (pfac_records_leftmost_longest_documents), shared by both tile
// passes and the write: at a position p of document d the candidate is the longest record at p that ends at or before
// off[d + 1].  Records at one position come in ascending length, so the ones that fit are a prefix of them: record i is
// the candidate iff it fits and the record behind it (at another position, or too long) does not.  Record i of the tile
// (heap index lo + i of c) -> pos, st, len, its document d; every lane takes part (the shuffles of final_len and
// doc_lookup), and lane 63 re-reads the record behind its chunk for the length and fit of that one.
template <int BYTES>
__device__ __forceinline__ bool ll_doc_candidate(const void *rec, unsigned long long lo, unsigned c, unsigned i,
                                                 unsigned long long cap, unsigned long long t, const short *flen, int freg,
                                                 bool fsmall, const DocWin &w, const unsigned long long *off, int lane,
                                                 unsigned &pos, unsigned &st, int &len, unsigned long long &d) {
    const bool have = i < c && lo + i < cap, hn = i + 1 < c && lo + i + 1 < cap;
    pos = 0;
    st = 0;
    if (have) heap_record<BYTES>(rec, lo + i, t, pos, st);
    unsigned pn = __shfl(pos, (lane + 1) & (WAVE - 1), WAVE), sn = __shfl(st, (lane + 1) & (WAVE - 1), WAVE);
    if (lane == WAVE - 1 && hn) heap_record<BYTES>(rec, lo + i + 1, t, pn, sn);
    len = final_len(flen, freg, fsmall, have, st);
    const int ln = final_len(flen, freg, fsmall, hn, sn);
    unsigned long long base, end;
    doc_lookup(w, off, have, pos, d, base, end);
    const bool fit = have && len > 0 && (unsigned long long)pos + (unsigned)len <= end;
    const bool next_fits = hn && pn == pos && ln > 0 && (unsigned long long)pn + (unsigned)ln <= end;   // (same document)
    return fit && !next_fits;
}

// DOCS: the per-document selection.  The candidate of a position is ll_doc_candidate's; a record's document comes from
// the tile's document window (lane j of every wave holds [dlo, dhi] of tile 64g + j).  The function pass also checks
// the offsets (as pfac_seg_count_kernel does) into *bad.  No candidate crosses a document end, so the chain restarts
// at every document by itself.
template <int BYTES, bool MARK, bool DOCS = false>
__global__ void __launch_bounds__(LL_WAVES * WAVE)
pfac_ll_tiles_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                     unsigned long long n_owned, const short *flen, unsigned num_final, unsigned M,
                     unsigned short *gfun, const unsigned short *gentry, unsigned long long *bits, unsigned *tcnt,
                     unsigned long long *gsum, const unsigned long long *off, unsigned long long n_docs,
                     unsigned long long *bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned g = blockIdx.x, M1 = M + 1, FS = ll_fun_stride(M1);
    unsigned short *cpos = reinterpret_cast<unsigned short *>(smem + w * LL_WAVE_LDS);   // tile offset of candidate k
    unsigned short *nxt = cpos + WTILE;                                                  // next[k]
    unsigned short *ends = nxt + WTILE;                                                  // pos + len, then exitE[k]
    unsigned *bm = reinterpret_cast<unsigned *>(ends);                                   // MARK: selected positions
    unsigned short *fslot = reinterpret_cast<unsigned short *>(smem + LL_WAVES * LL_WAVE_LDS);   // F of each wave's tile
    unsigned short *G = fslot + LL_WAVES * FS;                                           // !MARK: the running group function
    unsigned long long *tail = reinterpret_cast<unsigned long long *>(G + FS);           // MARK: tile entries, cursor, sums
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    if (!MARK)
        for (unsigned e = threadIdx.x; e < M1; e += blockDim.x) G[e] = (unsigned short)e;
    if (MARK && threadIdx.x == 0) tail[LL_WAVES] = gentry[g];
    unsigned long long wsel = 0;                                // selected records of this wave's tiles
    unsigned long long tdlo = 0, tdhi = 0;                      // DOCS: documents of tile 64g + lane
    if constexpr (DOCS) {
        if constexpr (!MARK) offsets_rule(GRID_THREAD, GRID_THREADS, off, n_docs, n_owned, bad);
        const unsigned long long tl = (unsigned long long)g * XGROUP + (unsigned)lane;
        unsigned long long ds, de;
        if (tl < n_tiles) tile_docs(off, n_docs, tl, n_tiles, ds, de, tdlo, tdhi);
    }
    __syncthreads();
    for (unsigned b = 0; b < (unsigned)XGROUP; b += LL_WAVES) {
        const unsigned long long t = (unsigned long long)g * XGROUP + b + w;
        const bool live = t < n_tiles;                          // (wave-uniform)
        unsigned K = 0, tend = 0;                               // candidates; the tile's end (a dead tile: identity)
        if (live) {
            const unsigned long long e = tix[t];
            const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
            const unsigned long long lo = e & TIX_BASE_MASK;
            const unsigned tb = (unsigned)(t * WTILE);
            tend = t + 1 == n_tiles ? (unsigned)(n_owned - t * WTILE) : (unsigned)WTILE;
            DocWin dw{};
            if constexpr (DOCS)
                if (c) dw = doc_window(off, __shfl(tdlo, (int)(b + w), WAVE), __shfl(tdhi, (int)(b + w), WAVE), lane);
            for (unsigned c0 = 0; c0 < c; c0 += WAVE) {
                const unsigned i = c0 + (unsigned)lane;
                unsigned pos = 0, st = 0;
                int len;
                bool cand;
                if constexpr (DOCS) {
                    unsigned long long d;
                    cand = ll_doc_candidate<BYTES>(rec, lo, c, i, cap, t, flen, freg, fsmall, dw, off, lane, pos, st, len, d);
                } else {
                    const bool have = i < c && lo + i < cap;
                    unsigned pn = 0, sn = 0;
                    if (have) heap_record<BYTES>(rec, lo + i, t, pos, st);
                    pn = __shfl(pos, (lane + 1) & (WAVE - 1), WAVE);
                    if (lane == WAVE - 1 && i + 1 < c && lo + i + 1 < cap) heap_record<BYTES>(rec, lo + i + 1, t, pn, sn);
                    len = final_len(flen, freg, fsmall, have, st);
                    cand = have && (i + 1 >= c || pn != pos) && len > 0;   // the last (longest) record at pos
                }
                const unsigned long long bal = __ballot(cand);
                const unsigned k = K + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
                if (cand && k < (unsigned)WTILE) {             // (positions are distinct: at most 4096 candidates)
                    cpos[k] = (unsigned short)(pos - tb);
                    ends[k] = (unsigned short)(pos - tb + (unsigned)len);
                }
                K = min(K + (unsigned)__popcll(bal), (unsigned)WTILE);
            }
            wave_lds_sync();
            for (int ch = (int)((K + WAVE - 1) / WAVE) - 1; ch >= 0; ch--) {
                const unsigned base = (unsigned)ch * WAVE, k = base + (unsigned)lane;
                const bool v = k < K;
                unsigned nx = K, E = 0;
                if (v) {
                    E = ends[k];
                    nx = ll_lower_bound(cpos, k + 1, min(k + (E - cpos[k]), K), E);
                }
                // (J, X, E): the chain goes on at in-chunk node J, or (J = 64) it left the chunk at candidate X (K: the
                // tile), E the end of its last pick inside the chunk
                unsigned J = v && nx < K && nx - base < (unsigned)WAVE ? nx - base : (unsigned)WAVE, X = nx;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    const int src = J < (unsigned)WAVE ? (int)J : lane;
                    const unsigned J2 = __shfl(J, src, WAVE), X2 = __shfl(X, src, WAVE), E2 = __shfl(E, src, WAVE);
                    if (J < (unsigned)WAVE) { J = J2; X = X2; E = E2; }
                }
                if (v) {
                    const unsigned ex = X < K ? ends[X] : E;    // X lies in a later chunk: its exitE is final
                    ends[k] = (unsigned short)ex;
                    nxt[k] = (unsigned short)nx;
                }
                wave_lds_sync();
            }
        }
        // F(e): the end of the chain of the first candidate at offset e or later (candidates at offsets <= M are among
        // the first M + 1), relative to the tile's end
        unsigned short *F = fslot + w * FS;
        for (unsigned e = (unsigned)lane; e < M1; e += WAVE) {
            const unsigned k = ll_lower_bound(cpos, 0, min(K, M1), e);
            const unsigned c = k < K ? (unsigned)ends[k] : e;
            F[e] = (unsigned short)min(c > tend ? c - tend : 0u, M);     // (<= M for lengths that fit the table)
        }
        __syncthreads();
        if (!MARK) {
            for (unsigned e = threadIdx.x; e < M1; e += blockDim.x) {
                unsigned v = G[e];
#pragma unroll
                for (int ww = 0; ww < LL_WAVES; ww++) v = fslot[ww * FS + v];
                G[e] = (unsigned short)v;
            }
        } else {
            if (threadIdx.x == 0) {
                unsigned v = (unsigned)tail[LL_WAVES];
                for (int ww = 0; ww < LL_WAVES; ww++) { tail[ww] = v; v = fslot[ww * FS + v]; }
                tail[LL_WAVES] = v;
            }
            __syncthreads();
            if (live) {
                for (unsigned i = (unsigned)lane; i < (unsigned)WTILE / 32; i += WAVE) bm[i] = 0u;   // (ends is dead now)
                wave_lds_sync();
                unsigned T = ll_lower_bound(cpos, 0, min(K, M1), (unsigned)tail[w]);
                unsigned sel = 0;
                while (T < K) {                                 // the chunk holding T: mark its part of the chain
                    const unsigned base = T & ~(unsigned)(WAVE - 1), k = base + (unsigned)lane;
                    const bool v = k < K;
                    const unsigned nx = v ? (unsigned)nxt[k] : K;
                    unsigned Jl[6];                             // in-chunk node 2^l steps on (64: left the chunk)
                    Jl[0] = v && nx < K && nx - base < (unsigned)WAVE ? nx - base : (unsigned)WAVE;
#pragma unroll
                    for (int l = 1; l < 6; l++) {
                        const unsigned p = Jl[l - 1];
                        const unsigned q = __shfl(p, p < (unsigned)WAVE ? (int)p : lane, WAVE);
                        Jl[l] = p < (unsigned)WAVE ? q : (unsigned)WAVE;
                    }
                    // the chain's furthest node <= lane (nodes increase along it): lane is on it iff that is lane;
                    // and its last node in the chunk
                    unsigned x = T - base, L = T - base;
#pragma unroll
                    for (int l = 5; l >= 0; l--) {
                        const unsigned y = __shfl(Jl[l], (int)x, WAVE), z = __shfl(Jl[l], (int)L, WAVE);
                        if (y <= (unsigned)lane) x = y;
                        if (z < (unsigned)WAVE) L = z;
                    }
                    const bool on = v && x == (unsigned)lane;
                    if (on) {
                        const unsigned p = cpos[k];
                        atomicOr(&bm[p >> 5], 1u << (p & 31u));
                    }
                    sel += (unsigned)__popcll(__ballot(on));
                    T = __shfl(nx, (int)L, WAVE);
                }
                wave_lds_sync();
                bits[t * (WTILE / 64) + lane] = (unsigned long long)bm[2 * lane] | ((unsigned long long)bm[2 * lane + 1] << 32);
                if (lane == 0) tcnt[t] = sel;
                wsel += sel;
            }
        }
        __syncthreads();
    }
    if (!MARK) {
        for (unsigned e = threadIdx.x; e < FS; e += blockDim.x) gfun[(unsigned long long)g * FS + e] = e < M1 ? G[e] : 0;
    } else {
        if (lane == 0) tail[LL_WAVES + 1 + w] = wsel;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int ww = 0; ww < LL_WAVES; ww++) s += tail[LL_WAVES + 1 + ww];
            gsum[g] = s;
        }
    }
}
#undef GRID_THREAD
#undef GRID_THREADS

// out[b] = fun[f1 - 1] o ... o fun[f0] for [f0, f1) = block b's `per` functions (blockDim >= M + 1: one entry each)
__global__ void pfac_ll_compose_kernel(const unsigned short *fun, unsigned M1, unsigned n, unsigned per, unsigned short *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short *buf = reinterpret_cast<unsigned short *>(smem);
    const unsigned FS = ll_fun_stride(M1), nfc = (unsigned)(LL_CHUNK_BYTES / 2) / FS;
    const unsigned f0 = blockIdx.x * per, f1 = min(f0 + per, n);
    unsigned v = threadIdx.x;
    for (unsigned a = f0; a < f1; a += nfc) {
        const unsigned m = min(nfc, f1 - a);
        __syncthreads();
        for (unsigned i = threadIdx.x; i < m * FS / 8; i += blockDim.x)
            reinterpret_cast<uint4 *>(buf)[i] = reinterpret_cast<const uint4 *>(fun + (unsigned long long)a * FS)[i];
        __syncthreads();
        if (threadIdx.x < M1)
            for (unsigned j = 0; j < m; j++) v = buf[j * FS + v];
    }
    if (threadIdx.x < FS) out[(unsigned long long)blockIdx.x * FS + threadIdx.x] = threadIdx.x < M1 ? (unsigned short)v : 0;
}

// block b: x = start[b] (start NULL: entry); for i in its [f0, f1): at[i] = x, x = fun[i](x).  The block that holds the
// last function stores the final x in *last (when last is not NULL).  The walk itself runs over LDS.
__global__ void pfac_ll_walk_kernel(const unsigned short *fun, unsigned M1, unsigned n, unsigned per, const unsigned short *start,
                                    unsigned entry, unsigned short *at, unsigned long long *last) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short *buf = reinterpret_cast<unsigned short *>(smem);
    const unsigned FS = ll_fun_stride(M1), nfc = (unsigned)(LL_CHUNK_BYTES / 2) / FS;
    const unsigned f0 = blockIdx.x * per, f1 = min(f0 + per, n);
    unsigned x = start ? start[blockIdx.x] : entry;
    for (unsigned a = f0; a < f1; a += nfc) {
        const unsigned m = min(nfc, f1 - a);
        __syncthreads();
        for (unsigned i = threadIdx.x; i < m * FS / 8; i += blockDim.x)
            reinterpret_cast<uint4 *>(buf)[i] = reinterpret_cast<const uint4 *>(fun + (unsigned long long)a * FS)[i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (unsigned j = 0; j < m; j++) { at[a + j] = (unsigned short)x; x = buf[j * FS + x]; }
    }
    if (threadIdx.x == 0 && last && f1 == n) *last = x;
}

// selected records -> out[k] = {pos, state} at their sorted index k (one wave per group of 64 tiles)
template <int BYTES>
__global__ void pfac_ll_write_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                     const unsigned long long *bits, const unsigned *tcnt, const unsigned long long *gpre,
                                     unsigned n_groups, pfac_record *out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    const unsigned kc = t < n_tiles ? tcnt[t] : 0u;
    const unsigned long long off0 = gpre[g] + (wave_incl_scan(kc) - kc);   // sorted index of the tile's first pick
    for (int j = 0; j < XGROUP; j++) {
        if (__shfl(kc, j, WAVE) == 0) continue;
        const unsigned long long tj = (unsigned long long)g * XGROUP + j;
        const unsigned tc = __shfl(c, j, WAVE);
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        const unsigned long long *tb = bits + tj * (WTILE / 64);
        unsigned long long k = __shfl(off0, j, WAVE);
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0, pn = 0, sn = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, tj, pos, st);
            pn = __shfl(pos, (lane + 1) & (WAVE - 1), WAVE);
            if (lane == WAVE - 1 && i + 1 < tc && tlo + i + 1 < cap) heap_record<BYTES>(rec, tlo + i + 1, tj, pn, sn);
            const unsigned p = pos - (unsigned)(tj * WTILE);
            const bool sel = have && (i + 1 >= tc || pn != pos) && ((tb[p >> 6] >> (p & 63u)) & 1ull);
            const unsigned long long bal = __ballot(sel);
            if (sel) {
                pfac_record o;
                o.pos = pos;
                o.state = st;
                out[k + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = o;
            }
            k += (unsigned)__popcll(bal);
        }
    }
}

// The per-document selection's write (one wave per group of 64 tiles): a record is written when it is the candidate
// under ll_doc_candidate's rule and its position bit is set, at its tile's prefix plus a ballot rank, as {pos, state}
// with pos relative to the scan.  doc_first[d] for every document d that starts in the tile = the tile's prefix plus
// the picks of the tile in front of off[d] (a pick of document d' < d lies before off[d], one of d' >= d at or after
// it): a popcount over the tile's bitmap, every lane one document, so no lane walks a run of documents.
template <int BYTES>
__global__ void pfac_ll_doc_write_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles,
                                         unsigned long long cap, const unsigned long long *off, unsigned long long n_docs,
                                         const short *flen, unsigned num_final, const unsigned long long *bits,
                                         const unsigned *tcnt, const unsigned long long *gpre, unsigned n_groups,
                                         pfac_record *out, unsigned long long *doc_first) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const bool fsmall = num_final <= (unsigned)WAVE;
    const int freg = fsmall && (unsigned)lane < num_final ? (int)flen[lane] : 0;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    const unsigned kc = t < n_tiles ? tcnt[t] : 0u;
    const unsigned long long off0 = gpre[g] + (wave_incl_scan(kc) - kc);   // sorted index of the tile's first pick
    unsigned long long ds = 0, de = 0, dlo = 0, dhi = 0;
    if (t < n_tiles) tile_docs(off, n_docs, t, n_tiles, ds, de, dlo, dhi);
    for (int j = 0; j < XGROUP; j++) {
        const unsigned long long tj = (unsigned long long)g * XGROUP + j;
        if (tj >= n_tiles) break;
        const unsigned kt = __shfl(kc, j, WAVE);
        const unsigned long long k0 = __shfl(off0, j, WAVE);
        const unsigned long long *tb = bits + tj * (WTILE / 64);
        if (kt) {
            const unsigned tc = __shfl(c, j, WAVE);
            const unsigned long long tlo = __shfl(lo, j, WAVE);
            const DocWin w = doc_window(off, __shfl(dlo, j, WAVE), __shfl(dhi, j, WAVE), lane);
            unsigned long long k = k0;
            for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
                unsigned pos, st;
                int len;
                unsigned long long d;
                const bool cand = ll_doc_candidate<BYTES>(rec, tlo, tc, c0 + (unsigned)lane, cap, tj, flen, freg, fsmall, w,
                                                          off, lane, pos, st, len, d);
                const unsigned p = pos - (unsigned)(tj * WTILE);
                const bool sel = cand && ((tb[p >> 6] >> (p & 63u)) & 1ull);
                const unsigned long long bal = __ballot(sel);
                if (sel) {
                    pfac_record o;
                    o.pos = pos;
                    o.state = st;
                    out[k + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = o;
                }
                k += (unsigned)__popcll(bal);
            }
        }
        const unsigned long long tds = __shfl(ds, j, WAVE), tde = __shfl(de, j, WAVE);
        if (tds < tde) {
            const unsigned long long bw = kt ? tb[lane] : 0ull;       // picks at tile offsets 64 lane .. 64 lane + 63
            const unsigned pc = (unsigned)__popcll(bw), below = wave_incl_scan(pc) - pc;
            for (unsigned long long d0 = tds; d0 < tde; d0 += WAVE) {
                const unsigned long long dd = d0 + (unsigned)lane;
                const bool v = dd < tde;
                const unsigned long long x = v ? off[dd] - tj * WTILE : 0ull;   // in [0, 4096] (checked offsets)
                const unsigned o = (unsigned)min(x, (unsigned long long)WTILE);
                const int wi = (int)min(o >> 6, 63u);
                const unsigned long long m = o >= (unsigned)WTILE ? ~0ull : (1ull << (o & 63u)) - 1ull;
                const unsigned long long wbits = __shfl(bw, wi, WAVE);
                const unsigned cnt = __shfl(below, wi, WAVE) + (unsigned)__popcll(wbits & m);
                if (v) doc_first[dd] = k0 + cnt;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Find-and-replace over the leftmost-longest selection (pfac_replace_leftmost_longest).  Picks (p_k, s_k) of the slot's
// last selection, L_k = flen[s_k], R_k = the replacement of s_k; c_{-1} = entry, c_k = p_k + L_k.  Segment k < n is the
// input gap [c_{k-1}, p_k) followed by R_k; segment n is the gap [c_{n-1}, n_owned) (empty when c_{n-1} >= n_owned).
// Segment k starts at output offset O_k = c_{k-1} - entry + D_k, D_k = sum_{j<k} (R_j - L_j).
//   pfac_rp_count_kernel     one workgroup per 1024 picks: per block of 64 picks X[b] = O_{64b} minus the group's
//                            prefix; the group's delta sum; checks the selection against the table and the scan
//   pfac_scan_groups_kernel  the group prefixes and the total delta, which give out_bytes on the host
//   pfac_rp_write_kernel     output-driven: each wave owns `wins` windows of 1 KiB, one 16-B chunk per lane.  The block
//                            that holds a byte is found by a 64-ary search over O_{64b} (ballot over 64 probes per
//                            round); a block's 64 segment offsets are rebuilt with a wave prefix into LDS; each lane
//                            merges the pieces of its chunk in registers and stores it with one dwordx4.
// Blocks whose segments are all empty (deletions with no gap between them) are never loaded: after a block the next
// one is found by galloping from it, so a window costs its bytes times a log factor, whatever collapses into it.
// With replacement templates (pfac_table_set_replacement_templates) a quoting state's segment is its gap, R[:split],
// the matched input bytes [p_k, p_k + L_k), then R[split:], and D_k sums R_j - L_j [j plain].  The match extraction
// (pfac_extract_leftmost_longest) is the same write with every gap empty and no segment n.

constexpr int RP_BLOCK = 64;                        // picks per block (one wave)
constexpr int RP_GROUP = 16;                        // blocks per workgroup of the count kernel (1024 picks)
constexpr int RP_WIN = 16 * WAVE;                   // output bytes per window (16 per lane)
constexpr int RP_WAVES = 4;                         // waves per workgroup of the write kernel

__device__ __forceinline__ unsigned long long wave_incl_scan64(unsigned long long x) {
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long t = __shfl_up(x, (unsigned)d, WAVE);
        if (lane >= d) x += t;
    }
    return x;
}

// The end of a count kernel (replace, gather), behind the waves' sums of their blocks in bsum[]: X[b] = first(lb) + the
// sums of the group's blocks in front of block b (lb: its index in the group), and the group's sum.
template <typename First>
__device__ __forceinline__ void rp_count_out(const unsigned long long *bsum, unsigned long long nb, unsigned long long *X,
                                             unsigned long long *gsum, First first) {
    __syncthreads();
    if (threadIdx.x < RP_GROUP) {
        const unsigned long long b = (unsigned long long)blockIdx.x * RP_GROUP + threadIdx.x;
        unsigned long long pre = 0;
        for (unsigned j = 0; j < threadIdx.x; j++) pre += bsum[j];
        if (b < nb) X[b] = first(threadIdx.x) + pre;
        if (threadIdx.x == RP_GROUP - 1) gsum[blockIdx.x] = pre + bsum[RP_GROUP - 1];
    }
}

// One wave per block of 64 items of size x (pick k's delta, id k's length): out[k] = base + the sizes in front of k in
// the block, and behind the last item out[n] = the total.
__device__ __forceinline__ void rp_block_offsets(unsigned long long base, unsigned long long x, unsigned long long k,
                                                 unsigned long long n, unsigned long long *out) {
    const unsigned long long incl = base + wave_incl_scan64(x);
    if (k < n) out[k] = incl - x;
    if (k + 1 == n) out[n] = incl;
}

// The three kernels are templates on <TEMPLATES, GAPS>.  TEMPLATES: some state quotes its match (split[s] !=
// PFAC_TEMPLATE_PLAIN: the pick becomes R[:split] + input[p, p + L) + R[split:], so its delta is R, not R - L).  GAPS
// false is the extraction (pfac_extract_leftmost_longest): the same segments without their gaps and without the tail,
// so a pick's "delta" is its whole length E_k and O_k is the sum of the lengths before it.  <false, true> is the plain
// replace: none of the code below that names split or tests GAPS is in it.
template <bool TEMPLATES, bool GAPS>
__global__ void __launch_bounds__(RP_GROUP / 4 * WAVE)
pfac_rp_count_kernel(const pfac_record *sel, unsigned long long n, unsigned long long entry, unsigned long long n_owned,
                     const short *flen, const unsigned *roff, unsigned num_final, unsigned long long *X,
                     unsigned long long *gsum, unsigned long long *res, const unsigned *split) {
    __shared__ unsigned long long bsum[RP_GROUP];
    __shared__ unsigned long long cst[RP_GROUP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = (n + RP_BLOCK - 1) / RP_BLOCK;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned lb = (unsigned)w * 4 + (unsigned)i;
        const unsigned long long b = (unsigned long long)blockIdx.x * RP_GROUP + lb;
        const unsigned long long k = b * RP_BLOCK + (unsigned)lane;
        const bool v = k < n;
        unsigned long long p = 0, end = 0, d = 0;
        if (v) {
            const pfac_record r = sel[k];
            p = r.pos;
            if (r.state < num_final) {
                const int L = flen[r.state];
                const unsigned R = roff[r.state + 1] - roff[r.state];
                end = p + (unsigned long long)(L > 0 ? L : 0);
                if constexpr (!TEMPLATES && GAPS) {
                    d = (unsigned long long)((long long)R - (long long)L);   // (two's complement: sums wrap correctly)
                } else {
                    bool quote = false;
                    if constexpr (TEMPLATES) quote = split[r.state] != PFAC_TEMPLATE_PLAIN;
                    const long long M = quote && L > 0 ? (long long)L : 0ll;     // the quoted bytes
                    d = (unsigned long long)(GAPS ? (long long)R - (long long)L + M : (long long)R + M);
                }
                bad |= L < 1;
            } else {
                bad = true;
            }
            bad |= p >= n_owned;
        }
        unsigned long long prev = __shfl_up(end, 1u, WAVE);
        if (lane == 0) {
            prev = entry;
            if (v && k > 0) {
                const pfac_record r = sel[k - 1];
                if (r.state < num_final) {
                    const int L = flen[r.state];
                    prev = (unsigned long long)r.pos + (unsigned long long)(L > 0 ? L : 0);
                }
            }
        }
        if (v) {
            bad |= p < prev;
            if (k + 1 == n) res[1] = end;                  // c_{n-1}
        }
        const unsigned long long s = wave_sum64(d);
        if (lane == 0) { bsum[lb] = s; cst[lb] = prev; }
    }
    if (__ballot(bad) && lane == 0) atomicOr(&res[0], 1ull);
    rp_count_out(bsum, nb, X, gsum, [&](unsigned lb) { return GAPS ? cst[lb] - entry : 0ull; });
}

// O_{64b}: the output offset of block b's first segment (b < nb)
__device__ __forceinline__ unsigned long long rp_block_out(const unsigned long long *X, const unsigned long long *gpre,
                                                           unsigned long long b) {
    return b == 0 ? 0ull : X[b] + gpre[b / RP_GROUP];
}

// the last block b in [lo, nb) with O_{64b} <= x, given O_{64 lo} <= x (wave-uniform): gallop, then narrow, 64 probes a round
__device__ unsigned long long rp_find(const unsigned long long *X, const unsigned long long *gpre, unsigned long long nb,
                                      unsigned long long lo, unsigned long long x) {
    const int lane = threadIdx.x & (WAVE - 1);
    unsigned long long stride = 1;
    for (;;) {
        const unsigned long long idx = lo + (unsigned long long)(lane + 1) * stride;
        const bool t = idx < nb && rp_block_out(X, gpre, idx) <= x;
        const unsigned c = (unsigned)__popcll(__ballot(t));
        if (c < (unsigned)WAVE) { lo += c * stride; break; }
        lo += (unsigned long long)WAVE * stride;
        stride *= WAVE;
    }
    while (stride > 1) {                                    // the answer lies in [lo, lo + stride)
        stride /= WAVE;
        const unsigned long long idx = lo + (unsigned long long)(lane + 1) * stride;
        const bool t = idx < nb && rp_block_out(X, gpre, idx) <= x;
        lo += (unsigned)__popcll(__ballot(t)) * stride;
    }
    return lo;
}

// 16 bytes at buf[a, a + 16), aligned a; bytes outside [0, size) read as 0 (only the chunks at the ends take the slow path)
__device__ __forceinline__ uint4 rp_half(const unsigned char *buf, long long a, unsigned long long size) {
    if (a >= 0 && (unsigned long long)a + 16 <= size) return *reinterpret_cast<const uint4 *>(buf + a);
    unsigned v[4] = {0u, 0u, 0u, 0u};
    if (a + 16 > 0 && a < (long long)size) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const long long j = a + i;
            if (j >= 0 && (unsigned long long)j < size) v[i >> 2] |= (unsigned)buf[j] << (8 * (i & 3));
        }
    }
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// acc bytes [j0, j1) := buf[a + j0, a + j1) (a may lie before the buffer: only bytes inside it are needed)
__device__ __forceinline__ void rp_merge(uint4 &acc, const unsigned char *buf, long long a, unsigned long long size,
                                         unsigned j0, unsigned j1) {
    const unsigned sh = (unsigned)(a & 15);
    const long long a0 = a - (long long)sh;
    const uint4 h0 = rp_half(buf, a0, size);
    const uint4 h1 = sh ? rp_half(buf, a0 + 16, size) : make_uint4(0u, 0u, 0u, 0u);
    const unsigned q = sh >> 2, r = sh & 3;
    const unsigned e0 = q == 0 ? h0.x : q == 1 ? h0.y : q == 2 ? h0.z : h0.w;
    const unsigned e1 = q == 0 ? h0.y : q == 1 ? h0.z : q == 2 ? h0.w : h1.x;
    const unsigned e2 = q == 0 ? h0.z : q == 1 ? h0.w : q == 2 ? h1.x : h1.y;
    const unsigned e3 = q == 0 ? h0.w : q == 1 ? h1.x : q == 2 ? h1.y : h1.z;
    const unsigned e4 = q == 0 ? h1.x : q == 1 ? h1.y : q == 2 ? h1.z : h1.w;
    const unsigned v0 = __builtin_amdgcn_alignbyte(e1, e0, r), v1 = __builtin_amdgcn_alignbyte(e2, e1, r);
    const unsigned v2 = __builtin_amdgcn_alignbyte(e3, e2, r), v3 = __builtin_amdgcn_alignbyte(e4, e3, r);
    auto low = [](int m) -> unsigned { return m <= 0 ? 0u : m >= 4 ? 0xffffffffu : (1u << (8 * m)) - 1u; };
    const unsigned m0 = low((int)j1) & ~low((int)j0), m1 = low((int)j1 - 4) & ~low((int)j0 - 4);
    const unsigned m2 = low((int)j1 - 8) & ~low((int)j0 - 8), m3 = low((int)j1 - 12) & ~low((int)j0 - 12);
    acc.x = (acc.x & ~m0) | (v0 & m0);
    acc.y = (acc.y & ~m1) | (v1 & m1);
    acc.z = (acc.z & ~m2) | (v2 & m2);
    acc.w = (acc.w & ~m3) | (v3 & m3);
}

// the last segment k in [0, h) with so[k] <= pos (so[0] <= pos)
__device__ __forceinline__ unsigned rp_segment(const unsigned long long *so, unsigned h, unsigned long long pos) {
    unsigned l = 0;
    while (h - l > 1) {
        const unsigned m = (l + h) >> 1;
        if (so[m] <= pos) l = m;
        else h = m;
    }
    return l;
}

// The output-driven loop of the write kernels (replace, gather): each wave owns `wins` windows of RP_WIN bytes, one
// 16-byte chunk at o per lane (lane `lane` of wave w of the workgroup).  b is the block of 64 segments at hand, cnt
// how many it has and [Ob, hi) the output bytes it covers: the caller's load_block(b, Ob, hi, cnt) puts block b's
// segments into the wave's LDS and sets the other three, and piece(cnt, acc, o, pos, e) merges into acc the run that
// starts at pos of the piece that holds it and returns its end (at most e).  rp_find gives the window's first block,
// and after a block the next one that is not empty.  A chunk is stored with one dwordx4; only the last partial 16 B of
// the whole output goes in pieces.  The block's state lives HERE, not in the kernels: handed in by reference it stays
// in memory until the loop is inlined into its kernel, behind the loop passes, and the kernels compile to other code
// than the parent's (DESIGN.md section 19 has the figures).
template <typename Load, typename Piece>
__device__ __forceinline__ void rp_write_windows(int lane, int w, const unsigned long long *X, const unsigned long long *gpre, unsigned long long nb,
                                                 unsigned long long out_bytes, unsigned wins, unsigned char *out,
                                                 Load load_block, Piece piece) {
    const unsigned long long A = ((unsigned long long)blockIdx.x * RP_WAVES + (unsigned)w) * wins * RP_WIN;
    if (A >= out_bytes) return;
    unsigned long long b = rp_find(X, gpre, nb, 0, A);
    unsigned long long Ob = 0, hi = 0;
    unsigned cnt = 0;
    load_block(b, Ob, hi, cnt);
    for (unsigned wi = 0; wi < wins; wi++) {
        const unsigned long long W = A + (unsigned long long)wi * RP_WIN;
        if (W >= out_bytes) break;
        const unsigned long long o = W + 16ull * (unsigned)lane;
        uint4 acc = make_uint4(0u, 0u, 0u, 0u);
        for (;;) {
            const unsigned long long e = min(o + 16, hi);
            unsigned long long pos = max(o, Ob);
            while (pos < e) pos = piece(cnt, acc, o, pos, e);
            if (hi >= W + RP_WIN || hi >= out_bytes) break;
            b = rp_find(X, gpre, nb, b + 1, hi);
            wave_lds_sync();                                    // (every lane is done with the old block)
            load_block(b, Ob, hi, cnt);
        }
        if (o + 16 <= out_bytes) {
            *reinterpret_cast<uint4 *>(out + o) = acc;
        } else if (o < out_bytes) {                             // the last partial 16 B of the whole output
            const unsigned m = (unsigned)(out_bytes - o);
            const unsigned v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if ((unsigned)(4 * i + 4) <= m) {
                    *reinterpret_cast<unsigned *>(out + o + 4 * i) = v[i];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if ((unsigned)(4 * i + j) < m) out[o + 4 * i + j] = (unsigned char)(v[i] >> (8 * j));
                }
            }
        }
    }
}

template <bool TEMPLATES, bool GAPS>
__global__ void __launch_bounds__(RP_WAVES * WAVE)
pfac_rp_write_kernel(const unsigned char *in, unsigned long long n_avail, const pfac_record *sel, unsigned long long n,
                     unsigned long long entry, const short *flen, const unsigned *roff, const unsigned char *rep,
                     unsigned long long rep_size, const unsigned long long *X, const unsigned long long *gpre,
                     unsigned long long out_bytes, unsigned wins, unsigned char *out, const unsigned *split) {
    __shared__ unsigned long long s_o[RP_WAVES][RP_BLOCK + 1];      // segment k's output offset (k = cnt: the tail entry)
    __shared__ unsigned long long s_src[RP_WAVES][RP_BLOCK + 1];    // c_{k-1}: where its gap starts in the input (no GAPS: p_k)
    __shared__ unsigned long long s_glen[GAPS ? RP_WAVES : 1][RP_BLOCK + 1];   // its gap's length
    __shared__ unsigned s_roff[RP_WAVES][RP_BLOCK];                 // its replacement's offset in rep
    __shared__ unsigned s_split[TEMPLATES ? RP_WAVES : 1][RP_BLOCK];   // TEMPLATES: the replacement bytes before the match (plain: R), ...
    __shared__ unsigned s_mlen[TEMPLATES ? RP_WAVES : 1][RP_BLOCK];    // ... and the quoted bytes (plain: 0)
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = n ? (n + RP_BLOCK - 1) / RP_BLOCK : 1;
    unsigned long long *so = s_o[w], *ssrc = s_src[w], *sgl = s_glen[GAPS ? w : 0];
    unsigned *sro = s_roff[w];
    unsigned *ssp = s_split[TEMPLATES ? w : 0], *sml = s_mlen[TEMPLATES ? w : 0];
    auto load_block = [&](unsigned long long b, unsigned long long &Ob, unsigned long long &hi, unsigned &cnt) {
        const unsigned long long k = b * RP_BLOCK + (unsigned)lane;
        const bool v = k < n;
        unsigned long long p = 0, end = 0;
        unsigned ro = 0, R = 0, sp = 0, M = 0;
        if (v) {
            const pfac_record r = sel[k];
            p = r.pos;
            end = p + (unsigned long long)flen[r.state];
            ro = roff[r.state];
            R = roff[r.state + 1] - ro;
            if constexpr (TEMPLATES) {
                sp = split[r.state];
                M = sp != PFAC_TEMPLATE_PLAIN ? (unsigned)(end - p) : 0u;
                sp = min(sp, R);                                // (plain: all of R stands before the empty match)
            }
        }
        unsigned long long prev = __shfl_up(end, 1u, WAVE);
        if (lane == 0) {
            prev = entry;
            if (b > 0) {
                const pfac_record r = sel[k - 1];
                prev = (unsigned long long)r.pos + (unsigned long long)flen[r.state];
            }
        }
        const unsigned long long G = GAPS && v ? p - prev : 0ull;
        const unsigned long long seg = v ? G + R + M : 0ull;
        const unsigned long long incl = wave_incl_scan64(seg);
        Ob = rp_block_out(X, gpre, b);
        cnt = (unsigned)min((unsigned long long)RP_BLOCK, n - min(n, b * RP_BLOCK));
        if (v) {
            so[lane] = Ob + incl - seg;
            ssrc[lane] = GAPS ? prev : p;                       // (either way the match starts at ssrc + G)
            if constexpr (GAPS) sgl[lane] = G;
            sro[lane] = ro;
            if constexpr (TEMPLATES) { ssp[lane] = sp; sml[lane] = M; }
        }
        const unsigned long long oT = Ob + (cnt ? __shfl(incl, (int)cnt - 1, WAVE) : 0ull);
        const unsigned long long cT = cnt ? __shfl(end, (int)cnt - 1, WAVE) : __shfl(prev, 0, WAVE);
        const bool last = b + 1 == nb;
        if (lane == 0) {
            so[cnt] = oT;
            ssrc[cnt] = cT;
            if constexpr (GAPS) sgl[cnt] = last ? out_bytes - oT : 0ull;
        }
        hi = last ? out_bytes : oT;                             // (no GAPS: no tail, the last block ends at out_bytes = oT)
        wave_lds_sync();
    };
    rp_write_windows(lane, w, X, gpre, nb, out_bytes, wins, out, load_block,
                     [&](unsigned cnt, uint4 &acc, unsigned long long o, unsigned long long pos, unsigned long long e) {
        const unsigned l = rp_segment(so, cnt + 1, pos);
        const unsigned long long gs = so[l], ge = GAPS ? gs + sgl[l] : gs;
        unsigned long long pe;
        if (GAPS && pos < ge) {                                 // the input gap
            pe = min(ge, e);
            rp_merge(acc, in, (long long)(ssrc[l] + o - gs), n_avail, (unsigned)(pos - o), (unsigned)(pe - o));
        } else if constexpr (!TEMPLATES) {                      // the replacement (l < cnt here)
            pe = min(so[l + 1], e);
            rp_merge(acc, rep, (long long)sro[l] + (long long)(o - ge), rep_size, (unsigned)(pos - o), (unsigned)(pe - o));
        } else {                                                // R[:split], the match as the caller wrote it, R[split:]
            const unsigned long long m0 = ge + ssp[l], m1 = m0 + sml[l];
            if (pos < m0) {
                pe = min(m0, e);
                rp_merge(acc, rep, (long long)sro[l] + (long long)(o - ge), rep_size, (unsigned)(pos - o), (unsigned)(pe - o));
            } else if (pos < m1) {
                pe = min(m1, e);
                rp_merge(acc, in, (long long)(ssrc[l] + (ge - gs)) + (long long)(o - m0), n_avail, (unsigned)(pos - o), (unsigned)(pe - o));
            } else {
                pe = min(so[l + 1], e);
                rp_merge(acc, rep, (long long)sro[l] + (long long)ssp[l] + (long long)(o - m1), rep_size, (unsigned)(pos - o), (unsigned)(pe - o));
            }
        }
        return pe;
    });
}

// Per-document output offsets (pfac_replace_documents), for a selection made from entry 0: out_off[d] = off[d] +
// D_{doc_first[d]}, D_k = sum_{j<k} (R_j - L_j).  Two kernels, O(n_picks + n_docs), no walk over a range:
//   pfac_rp_doc_delta_kernel    one wave per block of 64 picks: D_k for every pick, D[n] = the total.  The block's base
//                               comes from the count kernel: O_{64b} = c_{64b-1} + D_{64b} (entry 0).
//   pfac_rp_doc_offsets_kernel  one thread per document.
// Without GAPS (the extraction) D_k under the same definition is the output offset of pick k: the block's base is
// O_{64b} itself, no cursor subtracted, and D is the caller's pick offsets.
template <bool TEMPLATES, bool GAPS>
__global__ void __launch_bounds__(4 * WAVE)
pfac_rp_doc_delta_kernel(const pfac_record *sel, unsigned long long n, const short *flen, const unsigned *roff,
                         const unsigned long long *X, const unsigned long long *gpre, unsigned long long *D,
                         const unsigned *split) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long b = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6), k = b * RP_BLOCK + (unsigned)lane;
    if (b * RP_BLOCK >= n) return;
    unsigned long long dk = 0;
    if (k < n) {
        const pfac_record r = sel[k];
        if constexpr (!TEMPLATES && GAPS) {
            dk = (unsigned long long)((long long)(roff[r.state + 1] - roff[r.state]) - (long long)flen[r.state]);
        } else {
            bool quote = false;
            if constexpr (TEMPLATES) quote = split[r.state] != PFAC_TEMPLATE_PLAIN;
            const long long R = (long long)(roff[r.state + 1] - roff[r.state]), L = (long long)flen[r.state];
            dk = (unsigned long long)(R + (quote ? L : 0ll) - (GAPS ? L : 0ll));
        }
    }
    unsigned long long base = 0;                                // D_{64b}
    if (b > 0) {
        if constexpr (GAPS) {
            const pfac_record r = sel[b * RP_BLOCK - 1];
            base = X[b] + gpre[b / RP_GROUP] - ((unsigned long long)r.pos + (unsigned long long)flen[r.state]);
        } else {
            base = X[b] + gpre[b / RP_GROUP];
        }
    }
    rp_block_offsets(base, dk, k, n, D);
}

__global__ void pfac_rp_doc_offsets_kernel(const unsigned long long *off, const unsigned long long *doc_first,
                                           unsigned long long n_docs, const unsigned long long *D, unsigned long long n,
                                           unsigned long long *out_off) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
        const unsigned long long f = doc_first[d];
        out_off[d] = off[d] + (n ? D[f < n ? f : n] : 0ull);
    }
}

// ---------------------------------------------------------------------------
// GPU-side text emitter (replaces the fprintf loop of main.cc:335-350 on the device): the compact records of a scan ->
// the lines  "At position %4d, match pattern %d\n"  in output order, in one device buffer.  Three kernels: bytes per
// group of 64 tiles (line length depends on the digit counts), exclusive scan of the group sums (pfac_scan_groups_kernel),
// format.  The host only copies the finished text and write()s it.
__device__ __forceinline__ unsigned ndigits32(unsigned v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
__device__ __forceinline__ unsigned ndigits64(unsigned long long v) {       // v < 10^18
    return v < 1000000000ull ? ndigits32((unsigned)v) : 9u + ndigits32((unsigned)(v / 1000000000ull));
}
__device__ __forceinline__ unsigned text_line_len(unsigned long long pos, unsigned id) {
    const unsigned dp = ndigits64(pos);
    return 12u + (dp < 4u ? 4u : dp) + 16u + ndigits32(id) + 1u;
}
constexpr int TEXT_LINE_MAX = 12 + 18 + 16 + 10 + 1;          // positions below 10^18, ids below 2^32
constexpr int TEXT_IMG = 16 + WAVE * TEXT_LINE_MAX + 15;       // LDS image of one chunk of 64 lines, congruent mod 16 with its place in the text

// bytes of text per group of XGROUP tiles (lane j of a wave: tile g * 64 + j; its records by all lanes in turn)
template <int BYTES>
__global__ void pfac_text_size_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                      unsigned long long base, const int *idmap, unsigned long long *gsum, unsigned n_groups) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned long long total = 0;
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        unsigned long long sum = 0;
        for (unsigned i = (unsigned)lane; i < tc && tlo + i < cap; i += WAVE) {
            unsigned pos, st;
            heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            sum += text_line_len(base + pos, (unsigned)idmap[st]);
        }
        total += sum;                                          // (per lane; summed over the wave once, below)
    }
    total = wave_sum64(total);
    if (lane == 0) gsum[g] = total;
}

// decimal digits of v (nd of them, most significant first) to p[0..nd)
__device__ __forceinline__ void put_digits32(unsigned char *p, unsigned v, unsigned nd) {
    for (unsigned k = nd; k-- > 0;) { const unsigned q = v / 10u; p[k] = (unsigned char)('0' + (v - q * 10u)); v = q; }
}

template <int BYTES>
__global__ __launch_bounds__(256) void pfac_text_format_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tiles,
                                                               unsigned long long cap, unsigned long long base, const int *idmap,
                                                               const unsigned long long *gpre, unsigned n_groups, unsigned char *text) {
    __shared__ __attribute__((aligned(16))) unsigned char img_all[4][(TEXT_IMG + 15) / 16 * 16];
    const int lane = threadIdx.x & (WAVE - 1);
    unsigned char *img = img_all[threadIdx.x >> 6];
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned long long at = gpre[g];                           // text offset of the next line (wave-uniform)
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {           // a chunk of up to 64 lines
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0, id = 0, len = 0, dp = 0, di = 0;
            unsigned long long gp = 0;
            if (have) {
                heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
                id = (unsigned)idmap[st];
                gp = base + pos;
                dp = ndigits64(gp);
                di = ndigits32(id);
                len = 12u + (dp < 4u ? 4u : dp) + 16u + di + 1u;
            }
            const unsigned incl = wave_incl_scan(len);
            const unsigned total = bcast_last(incl);
            const unsigned a0 = (unsigned)(at & 15ull);        // the image starts at the 16-byte block the chunk's first byte lies in
            if (have) {
                unsigned char *p = img + a0 + (incl - len);
                const char *h = "At position ";
#pragma unroll
                for (int k = 0; k < 12; k++) p[k] = (unsigned char)h[k];
                p += 12;
                for (unsigned k = dp; k < 4u; k++) *p++ = ' ';                               // %4d
                if (gp < 1000000000ull) put_digits32(p, (unsigned)gp, dp);
                else {
                    const unsigned hi = (unsigned)(gp / 1000000000ull), lo9 = (unsigned)(gp - (unsigned long long)hi * 1000000000ull);
                    put_digits32(p, hi, dp - 9u);
                    put_digits32(p + (dp - 9u), lo9, 9u);
                }
                p += dp;
                const char *m = ", match pattern ";
#pragma unroll
                for (int k = 0; k < 16; k++) p[k] = (unsigned char)m[k];
                p += 16;
                put_digits32(p, id, di);
                p[di] = (unsigned char)'\n';
            }
            wave_lds_sync();
            // image bytes [a0, a0 + total) -> text[at, at + total): whole 16-byte blocks with one store per lane, the ragged
            // first and last block byte by byte (their other bytes belong to the neighbouring chunks)
            unsigned char *dst = text + (at - a0);            // 16-byte aligned (the text buffer is)
            const unsigned end = a0 + total;
            const unsigned b_lo = a0 ? 16u : 0u, b_hi = end & ~15u;   // full blocks cover [b_lo, b_hi)
            if (b_hi > b_lo) {
                for (unsigned o = b_lo + 16u * (unsigned)lane; o < b_hi; o += 16u * WAVE)
                    __builtin_nontemporal_store(*reinterpret_cast<const u32x4 *>(img + o), reinterpret_cast<u32x4 *>(dst + o));
                if (a0 && (unsigned)lane < 16u - a0) dst[a0 + lane] = img[a0 + lane];
                if ((unsigned)lane < end - b_hi) dst[b_hi + lane] = img[b_hi + lane];
            } else {
                // no whole block: at most 31 bytes (e.g. one short line): byte by byte
                if (a0 + (unsigned)lane < end) dst[a0 + lane] = img[a0 + lane];
            }
            wave_lds_sync();
            at += total;
        }
    }
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// byte i = byte (i & 7) (little endian) of splitmix64(seed + (i >> 3)); dst 8-B aligned, n rounded up by caller
__global__ void pfac_fill_random_kernel(unsigned long long *dst, unsigned long long n_words, unsigned long long seed) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride)
        dst[i] = splitmix64(seed + i);
}

// byte i = pat[(phase + i) % period]
__global__ void pfac_fill_tiled_kernel(unsigned char *dst, unsigned long long n, const unsigned char *pat,
                                       unsigned period, unsigned long long phase) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x * 16;
    for (unsigned long long i = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n; i += stride) {
        unsigned k = (unsigned)((phase + i) % period);
        if (i + 16 <= n) {
            union { unsigned char b[16]; uint4 v; } u;
#pragma unroll
            for (int j = 0; j < 16; j++) { u.b[j] = pat[k]; k = k + 1 == period ? 0 : k + 1; }
            *reinterpret_cast<uint4 *>(dst + i) = u.v;
        } else {
            for (unsigned long long j = i; j < n; j++) { dst[j] = pat[k]; k = k + 1 == period ? 0 : k + 1; }
        }
    }
}

// ---------------------------------------------------------------------------
// Document offsets from a delimiter (pfac_slot_doc_offsets_split): a document ends after every delimiter byte.  The
// shape of the other passes, over INPUT bytes: delimiters per 4 KiB tile (one wave per tile at a time, four dwordx4 loads
// per lane, the exact SWAR compare of root_mask<1>), sums per group of 64 tiles, pfac_scan_groups_kernel, then the same
// loads again and one 8-byte store per delimiter at its rank.  A tile word = delimiters in the tile | (1 + tile-local
// offset of its last delimiter, 0 if none) << 32: the maximum of those ends over the input is tail_start.

// The lane's 16 bytes at offset b of in[0, n): one dwordx4 load where the chunk lies inside the input; the chunk that
// holds byte n - 1 is read byte by byte, its bytes at or past n replaced by a value that is not the delimiter (pad_x4),
// and a chunk at or past n is all padding -- no byte at or past n is read, whatever the buffer holds there.
__device__ __forceinline__ u32x4 split_chunk(const unsigned char *in, unsigned long long b, unsigned long long n, unsigned pad_x4) {
    u32x4 w = {pad_x4, pad_x4, pad_x4, pad_x4};
    if (b + 16 <= n) {
        w = *reinterpret_cast<const u32x4 *>(in + b);
    } else if (b < n) {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (b + j < n) w[j >> 2] = (w[j >> 2] & ~(0xFFu << (8 * (j & 3)))) | ((unsigned)in[b + j] << (8 * (j & 3)));
    }
    return w;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long y = __shfl_xor(x, d, WAVE); x = y > x ? y : x; }
    return x;
}

__global__ void __launch_bounds__(256)
pfac_split_count_kernel(const unsigned char *in, unsigned long long n, unsigned long long n_tiles, unsigned delim_x4,
                        unsigned long long *tile) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    for (unsigned long long t = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); t < n_tiles; t += n_waves) {
        const unsigned long long base = t * WTILE + (unsigned)lane * 16u;
        u32x4 w[SUBS];
#pragma unroll
        for (int s = 0; s < SUBS; s++) w[s] = split_chunk(in, base + (unsigned)s * SUB, n, ~delim_x4);
        unsigned cnt = 0, last = 0;
#pragma unroll
        for (int s = 0; s < SUBS; s++) {
            const unsigned m = root_mask<1>(w[s], nullptr, delim_x4);
            cnt += (unsigned)__popc(m);
            if (m) last = (unsigned)s * SUB + (unsigned)lane * 16u + (32u - (unsigned)__clz(m));
        }
        const unsigned long long sum = wave_sum64(cnt), end = wave_max64(last);
        if (lane == 0) tile[t] = sum | (end << 32);
    }
}
// per group of 64 tiles: its delimiters, and the end (1 + offset in the input) of its last one (0 if none)
__global__ void pfac_split_group_kernel(const unsigned long long *tile, unsigned long long n_tiles, unsigned long long *gsum,
                                        unsigned long long *glast, unsigned n_groups) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tile[t] : 0ull;
    const unsigned long long sum = wave_sum64(e & 0xFFFFFFFFull);
    const unsigned long long end = wave_max64((e >> 32) ? t * WTILE + (e >> 32) : 0ull);
    if (lane == 0) { gsum[g] = sum; glast[g] = end; }
}
// behind the group prefix: res[0] = delimiters in the input, res[1] = the end of the last one = tail_start
__global__ void pfac_split_ends_kernel(const unsigned long long *gsum, const unsigned long long *glast, unsigned n_groups,
                                       unsigned long long *res) {                         // ONE block of 1024 threads
    __shared__ unsigned long long part[1024];
    unsigned long long m = 0;
    for (unsigned i = threadIdx.x; i < n_groups; i += 1024) { const unsigned long long v = glast[i]; m = v > m ? v : m; }
    part[threadIdx.x] = m;
    __syncthreads();
    for (unsigned d = 512; d >= 1; d >>= 1) {
        if (threadIdx.x < d) { const unsigned long long v = part[threadIdx.x + d]; if (v > part[threadIdx.x]) part[threadIdx.x] = v; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { res[0] = gsum[n_groups]; res[1] = part[0]; }
}
// off[1 + rank] = i + 1 for every delimiter in[i]; one lane writes off[0] = 0 and, for an unterminated last document, the
// closing off[close_at] = n (close_at 0: none).  A rank at or past `total` (the count pass's sum: the offsets buffer was
// sized from it) is never stored, so an input rewritten between the two passes costs wrong offsets, not a stray write.
__global__ void __launch_bounds__(256)
pfac_split_write_kernel(const unsigned char *in, unsigned long long n, unsigned long long n_tiles, unsigned delim_x4,
                        const unsigned long long *tile, const unsigned long long *gpre, unsigned long long total,
                        unsigned long long close_at, unsigned long long *off) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long wave0 = (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    if (wave0 == 0 && lane == 0) {
        off[0] = 0;
        if (close_at) off[close_at] = n;
    }
    for (unsigned long long t = wave0; t < n_tiles; t += n_waves) {
        const unsigned long long g = t / XGROUP, tl = g * XGROUP + lane;
        const int j = (int)(t % XGROUP);
        const unsigned c = tl < n_tiles ? (unsigned)tile[tl] : 0u;
        if (__shfl(c, j, WAVE) == 0) continue;                          // (wave-uniform: a tile without a delimiter is not read again)
        unsigned long long rank = gpre[g] + wave_sum64(lane < j ? c : 0u);
        const unsigned long long base = t * WTILE + (unsigned)lane * 16u;
        u32x4 w[SUBS];
#pragma unroll
        for (int s = 0; s < SUBS; s++) w[s] = split_chunk(in, base + (unsigned)s * SUB, n, ~delim_x4);
#pragma unroll
        for (int s = 0; s < SUBS; s++) {
            unsigned m = root_mask<1>(w[s], nullptr, delim_x4);
            const unsigned k = (unsigned)__popc(m), incl = wave_incl_scan(k);
            unsigned long long r = rank + (incl - k);
            rank += bcast_last(incl);
            const unsigned long long at = base + (unsigned)s * SUB + 1u;
            while (m) {
                const unsigned b = (unsigned)__ffs(m) - 1u;
                m &= m - 1u;
                if (r < total) off[1 + r] = at + b;
                r++;
            }
        }
    }
}

// The documents that hold (or lack) a match (pfac_documents_matching): an ordered stream compaction over the flags
// (doc_first[d + 1] > doc_first[d]) != invert.  One wave per group of 64 blocks of 64 documents, a ballot and a popcount
// per block; the count form leaves the group's sum, the write form starts at the group's prefix and stores document d at
// prefix + flags before it.  Like the split's write, no index at or past `total` is stored.
// The context form (pfac_documents_matching_context, grep -A / -B / -C) is the same compaction over another flag: doc_first
// is a prefix array, so "some document of [d - after, d + before] has a record" is doc_first[hi + 1] > doc_first[lo] with
// both ends clamped -- still two loads per document.  `before` and `after` arrive clamped to n_docs (d + before cannot wrap).
// The groups form (pfac_documents_matching_groups) is the third flag: the array holds a group mask per document (one
// load per document) and the three words are the predicate's sets, all_of / any_of / none_of.
// The scores forms (pfac_documents_matching_scores) are the fourth and fifth: the array holds a pfac_doc_score per
// document (one 16-byte load) judged against the windows of a pfac_score_rule; DM_DENSITY also loads the document's two
// offsets and compares score * den with num * length as two 128-bit products -- |score|, |num| <= 2^63 and den,
// length < 2^64, so each product lies inside (-2^127, 2^127) and the compare is exact.
constexpr int DM_BLOCKS = 64;
enum : int { DM_PLAIN = 0, DM_CONTEXT = 1, DM_GROUPS = 2, DM_SCORES = 3, DM_DENSITY = 4 };
template <bool WRITE, int PRED>
__device__ __forceinline__ void docs_matching_body(const unsigned long long *doc_first, unsigned long long n_docs, unsigned invert,
                                                   unsigned long long before, unsigned long long after, unsigned long long none_of,
                                                   unsigned long long *gsum, unsigned n_groups, unsigned long long total,
                                                   unsigned long long *ids, const pfac_score_rule *rule = nullptr,
                                                   const unsigned long long *off = nullptr) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long d0 = (unsigned long long)g * (DM_BLOCKS * WAVE);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long run = WRITE ? gsum[g] : 0ull;
#pragma unroll 4
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long d = d0 + (unsigned long long)b * WAVE + lane;
        const bool have = d < n_docs;
        bool flag;
        if (PRED == DM_SCORES || PRED == DM_DENSITY) {          // doc_first is the scores
            const ulonglong2 v = have ? reinterpret_cast<const ulonglong2 *>(doc_first)[d] : make_ulonglong2(0ull, 0ull);
            const long long sc = (long long)v.x;
            bool ok = v.y >= rule->min_count && v.y <= rule->max_count && sc >= rule->min_score && sc <= rule->max_score;
            if (PRED == DM_DENSITY) {
                const unsigned long long lo = have ? off[d] : 0ull, hi = have ? off[d + 1] : 0ull;
                ok = ok && (__int128)sc * (__int128)rule->density_den >= (__int128)rule->density_num * (__int128)(hi - lo);
            }
            flag = have && (ok != (invert != 0u));
        } else if (PRED == DM_GROUPS) {                                // before = all_of, after = any_of
            const unsigned long long m = have ? doc_first[d] : 0ull;
            const bool ok = (m & before) == before && (after == 0ull || (m & after) != 0ull) && (m & none_of) == 0ull;
            flag = have && (ok != (invert != 0u));
        } else if (PRED == DM_CONTEXT) {
            const unsigned long long first = d - (after < d ? after : d), last = d + before < n_docs ? d + before : n_docs - 1;
            const unsigned long long lo = have ? doc_first[first] : 0ull, hi = have ? doc_first[last + 1] : 0ull;
            flag = have && hi > lo;
        } else {
            const unsigned long long lo = have ? doc_first[d] : 0ull, hi = have ? doc_first[d + 1] : 0ull;
            flag = have && ((hi > lo) != (invert != 0u));
        }
        const unsigned long long mask = __ballot(flag);
        if (WRITE && flag) {
            const unsigned long long r = run + (unsigned long long)__popcll(mask & below);
            if (r < total) ids[r] = d;
        }
        run += (unsigned long long)__popcll(mask);
    }
    if (!WRITE && lane == 0) gsum[g] = run;
}
template <bool WRITE>
__global__ void __launch_bounds__(256)
pfac_docs_matching_kernel(const unsigned long long *doc_first, unsigned long long n_docs, unsigned invert, unsigned long long *gsum,
                          unsigned n_groups, unsigned long long total, unsigned long long *ids) {
    docs_matching_body<WRITE, DM_PLAIN>(doc_first, n_docs, invert, 0ull, 0ull, 0ull, gsum, n_groups, total, ids);
}
template <bool WRITE>
__global__ void __launch_bounds__(256)
pfac_docs_context_kernel(const unsigned long long *doc_first, unsigned long long n_docs, unsigned long long before,
                         unsigned long long after, unsigned long long *gsum, unsigned n_groups, unsigned long long total,
                         unsigned long long *ids) {
    docs_matching_body<WRITE, DM_CONTEXT>(doc_first, n_docs, 0u, before, after, 0ull, gsum, n_groups, total, ids);
}
template <bool WRITE>
__global__ void __launch_bounds__(256)
pfac_docs_groups_kernel(const unsigned long long *masks, unsigned long long n_docs, unsigned invert, unsigned long long all_of,
                        unsigned long long any_of, unsigned long long none_of, unsigned long long *gsum, unsigned n_groups,
                        unsigned long long total, unsigned long long *ids) {
    docs_matching_body<WRITE, DM_GROUPS>(masks, n_docs, invert, all_of, any_of, none_of, gsum, n_groups, total, ids);
}
template <bool WRITE, bool DENSITY>
__global__ void __launch_bounds__(256)
pfac_docs_scores_kernel(const pfac_doc_score *scores, unsigned long long n_docs, unsigned invert, pfac_score_rule rule,
                        const unsigned long long *off, unsigned long long *gsum, unsigned n_groups, unsigned long long total,
                        unsigned long long *ids) {
    docs_matching_body<WRITE, DENSITY ? DM_DENSITY : DM_SCORES>(reinterpret_cast<const unsigned long long *>(scores), n_docs, invert,
                                                                0ull, 0ull, 0ull, gsum, n_groups, total, ids, &rule, off);
}

// ---------------------------------------------------------------------------
// The k best documents by score or by count (pfac_documents_top_scores).  A document's key is mapped to a 64-bit word
// whose UNSIGNED ASCENDING order is the rank order (top_key): the count as it is, the score with its sign bit flipped,
// and all bits inverted for "largest first".  Three steps, none of which goes back to the host for a digit:
//   pfac_top_hist_kernel     TOP_PASSES times, most significant digit first: a grid-stride read of the pairs (and of the
//                            two offsets under a density); the candidates whose higher digits equal the prefix found so
//                            far are counted by their next digit -- the lanes of a wave that agree on the digit are
//                            found with ballots and ONE of them adds their number to the workgroup's 32-bit LDS
//                            partial; the non-zero partials go to the 64-bit histogram with no-return atomics.
//                            (TOP_COPIES histograms per pass, dealt to the workgroups round-robin).
//                            The digit that holds the rank is chosen by the first wave of EVERY WORKGROUP of the next
//                            pass from the small histograms (top_pick: 4 bins per lane, a scan over the lanes):
//                            prefix |= digit, krem -= the candidates in front of it; the first thread of the grid
//                            records that state (words of their own per pass: nobody reads what another writes in the
//                            same launch).  The first histograms' sum is n_cand, the word the host copies back:
//                            n_top = min(k, n_cand).  pfac_top_final_kernel, one wave, does the same behind the last
//                            pass: prefix = T, the key of rank n_top, and krem = need, the candidates with key T that
//                            are still to be taken
//   pfac_top_compact_kernel  the matching pass's compaction with TWO counts per block and group: candidates with key < T
//                            and with key == T.
//                            Document d is reported iff its key < T, or its key == T and fewer than `need` candidates
//                            with key T have a smaller id; it lands at (keys < T in front of it) + min(keys == T in
//                            front of it, need) -- ascending ids.  Unranked: the id and the pair are stored there.
//                            Ranked: the entry (key word, id) goes to the sort's first buffer
//   the sort                 (PFAC_TOP_RANKED) a stable LSD radix sort of the entries by the key word, TOP_PASSES
//                            passes.  Ascending ids in, a stable sort: ties end with the smaller id first.  An entry's
//                            rank among its wave's equal digits comes from the ballots (ts_rank) -- no atomic on the
//                            output.  n_top <= TS_BLOCK: pfac_top_sort_one_kernel, one workgroup, all passes through
//                            LDS.  Above: per pass pfac_top_sort_hist_kernel (digit counts per block of TS_BLOCK
//                            entries, digit-major, so ONE exclusive scan, pfac_scan_groups_kernel, gives every (digit,
//                            block) its base) and pfac_top_sort_scatter_kernel, ping-pong between two buffers.  The
//                            last pass writes the ids and gathers each winner's pair from the scores.
// Nothing is stored at or past n_top in either output.
constexpr int TOP_BITS = 8;
constexpr int TOP_BINS = 1 << TOP_BITS;
constexpr int TOP_PASSES = 64 / TOP_BITS;
constexpr int TOP_PER_LANE = TOP_BINS / WAVE;
constexpr int TOP_COPIES = 8;                                       // histograms per pass: workgroup b adds to copy b % 8 (an address takes
                                                                    // its atomics one at a time: 2048 workgroups on one would be the pass)
constexpr int TOP_STATE = TOP_PASSES * TOP_COPIES * TOP_BINS;       // behind the histograms: (prefix, krem) in front of pass p at
constexpr int TOP_NCAND = TOP_STATE + 2 * (TOP_PASSES + 1);         // TOP_STATE + 2 p (1 <= p <= TOP_PASSES), then the candidates
constexpr int TOP_WORK_WORDS = TOP_NCAND + 1;
constexpr int TS_ITEMS = 4;                                         // entries per thread of a sort block, ...
constexpr int TS_WAVES = 4;
constexpr int TS_BLOCK = TS_WAVES * WAVE * TS_ITEMS;                // ... which holds 1024: wave w owns [256 w, 256 w + 256)
static_assert(TS_BLOCK == PFAC_TOP_SORT_BLOCK, "the header names the sort's block size");
static_assert(TS_WAVES * WAVE == TOP_BINS, "one thread per digit in the histogram flush and the sort's bases");

__device__ __forceinline__ unsigned long long top_key(const ulonglong2 v, unsigned flags) {
    const unsigned long long w = (flags & PFAC_TOP_BY_COUNT) ? v.y : v.x ^ (1ull << 63);
    return (flags & PFAC_TOP_LOWEST) ? w : ~w;
}
// the rule of docs_matching_body's scores forms, for a document that exists (d < n_docs)
template <bool DENSITY>
__device__ __forceinline__ bool top_candidate(const ulonglong2 v, const pfac_score_rule &rule, unsigned invert,
                                              const unsigned long long *off, unsigned long long d) {
    const long long sc = (long long)v.x;
    bool ok = v.y >= rule.min_count && v.y <= rule.max_count && sc >= rule.min_score && sc <= rule.max_score;
    if (DENSITY) {
        const unsigned long long lo = off[d], hi = off[d + 1];
        ok = ok && (__int128)sc * (__int128)rule.density_den >= (__int128)rule.density_num * (__int128)(hi - lo);
    }
    return ok != (invert != 0u);
}
// match-any over the digit's bits: the `valid` lanes of the wave whose digit equals this lane's (called by the whole
// wave; the value of a lane without `valid` means nothing)
__device__ __forceinline__ unsigned long long wave_match_digit(unsigned digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < TOP_BITS; b++) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long s = __ballot(bit);
        m &= bit ? s : ~s;
    }
    return m;
}
// The state behind pass `pass` from the state in front of it and that pass's histogram (called by a whole wave; every
// lane gets the same values): the digit that holds rank krem.  In front of pass 0 the state is (0, k), and k clamps to
// the candidates, the histogram's sum (n_cand means that for pass 0 only).  krem == 0 (no candidate, or k == 0) picks
// nothing and stays 0.
__device__ __forceinline__ void top_pick(const unsigned long long *work, int pass, unsigned long long k, unsigned long long &prefix,
                                         unsigned long long &krem, unsigned long long &n_cand) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long *h = work + pass * (TOP_COPIES * TOP_BINS) + lane * TOP_PER_LANE;
    unsigned long long c[TOP_PER_LANE], sum = 0;
#pragma unroll
    for (int j = 0; j < TOP_PER_LANE; j++) {
        c[j] = 0ull;
#pragma unroll
        for (int i = 0; i < TOP_COPIES; i++) c[j] += h[i * TOP_BINS + j];
        sum += c[j];
    }
    unsigned long long incl = sum;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long y = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += y;
    }
    n_cand = __shfl(incl, WAVE - 1, WAVE);
    if (pass == 0) { prefix = 0ull; krem = k < n_cand ? k : n_cand; }
    else { prefix = work[TOP_STATE + 2 * pass]; krem = work[TOP_STATE + 2 * pass + 1]; }
    unsigned long long run = incl - sum;                            // candidates in front of this lane's digits
    const bool mine = krem > run && krem <= incl;                   // one lane (1 <= krem <= the sum), or none
    unsigned digit = (unsigned)lane * TOP_PER_LANE;
#pragma unroll
    for (int j = 0; j < TOP_PER_LANE - 1; j++) {
        if (krem > run + c[j]) { run += c[j]; digit++; }
        else break;
    }
    const unsigned long long who = __ballot(mine);
    if (who) {
        const int src = __ffsll((long long)who) - 1;
        prefix |= (unsigned long long)__shfl(digit, src, WAVE) << (64 - TOP_BITS * (pass + 1));
        krem = __shfl(krem - run, src, WAVE);
    }
}

template <bool DENSITY>
__global__ void __launch_bounds__(TOP_BINS)
pfac_top_hist_kernel(const pfac_doc_score *scores, unsigned long long n_docs, unsigned invert, pfac_score_rule rule,
                     const unsigned long long *off, unsigned flags, int pass, unsigned long long k, unsigned long long *work) {
    __shared__ unsigned part[TOP_BINS];
    __shared__ unsigned long long picked;
    part[threadIdx.x] = 0u;
    const int lane = threadIdx.x & (WAVE - 1);
    const int shift = 64 - TOP_BITS * (pass + 1);
    if (pass > 0 && threadIdx.x < WAVE) {                           // the first wave picks for the workgroup
        unsigned long long p, krem, n_cand;
        top_pick(work, pass - 1, k, p, krem, n_cand);
        if (threadIdx.x == 0) {
            picked = p;
            if (blockIdx.x == 0) {
                work[TOP_STATE + 2 * pass] = p;
                work[TOP_STATE + 2 * pass + 1] = krem;
                if (pass == 1) work[TOP_NCAND] = n_cand;
            }
        }
    }
    __syncthreads();
    const unsigned long long prefix = pass > 0 ? picked : 0ull;
    const unsigned long long stride = (unsigned long long)gridDim.x * TOP_BINS;
    for (unsigned long long d0 = (unsigned long long)blockIdx.x * TOP_BINS + (threadIdx.x & ~(WAVE - 1)); d0 < n_docs; d0 += stride) {
        const unsigned long long d = d0 + lane;                          // (d0 is wave-uniform: the ballots see all 64 lanes)
        const bool have = d < n_docs;
        const ulonglong2 v = have ? reinterpret_cast<const ulonglong2 *>(scores)[d] : make_ulonglong2(0ull, 0ull);
        const unsigned long long w = top_key(v, flags);
        bool cand = have && top_candidate<DENSITY>(v, rule, invert, off, d);
        if (pass > 0) cand = cand && ((w ^ prefix) >> (shift + TOP_BITS)) == 0ull;
        const unsigned digit = (unsigned)(w >> shift) & (TOP_BINS - 1u);
        const unsigned long long m = wave_match_digit(digit, cand);
        if (cand && lane == __ffsll((long long)m) - 1)
            __hip_atomic_fetch_add(part + digit, (unsigned)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    const unsigned c = part[threadIdx.x];
    if (c)
        __hip_atomic_fetch_add(work + (pass * TOP_COPIES + blockIdx.x % TOP_COPIES) * TOP_BINS + threadIdx.x, (unsigned long long)c,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// behind the last pass, ONE wave: T and need into the words "in front of pass TOP_PASSES"
__global__ void __launch_bounds__(WAVE)
pfac_top_final_kernel(unsigned long long *work, unsigned long long k) {
    unsigned long long T, need, n_cand;
    top_pick(work, TOP_PASSES - 1, k, T, need, n_cand);
    if (threadIdx.x == 0) {
        work[TOP_STATE + 2 * TOP_PASSES] = T;
        work[TOP_STATE + 2 * TOP_PASSES + 1] = need;
        if (TOP_PASSES == 1) work[TOP_NCAND] = n_cand;
    }
}

template <bool WRITE, bool DENSITY>
__global__ void __launch_bounds__(256)
pfac_top_compact_kernel(const pfac_doc_score *scores, unsigned long long n_docs, unsigned invert, pfac_score_rule rule,
                        const unsigned long long *off, unsigned flags, const unsigned long long *work, unsigned long long *bsum,
                        unsigned long long *esum, unsigned n_groups, unsigned long long total, unsigned long long *ids,
                        pfac_doc_score *top, ulonglong2 *ent) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long T = work[TOP_STATE + 2 * TOP_PASSES], need = work[TOP_STATE + 2 * TOP_PASSES + 1];
    const unsigned long long d0 = (unsigned long long)g * (DM_BLOCKS * WAVE);
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long run_b = WRITE ? bsum[g] : 0ull, run_e = WRITE ? esum[g] : 0ull;
#pragma unroll 4
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long d = d0 + (unsigned long long)b * WAVE + lane;
        const bool have = d < n_docs;
        const ulonglong2 v = have ? reinterpret_cast<const ulonglong2 *>(scores)[d] : make_ulonglong2(0ull, 0ull);
        const unsigned long long w = top_key(v, flags);
        const bool cand = have && top_candidate<DENSITY>(v, rule, invert, off, d);
        const bool before = cand && w < T, equal = cand && w == T;
        const unsigned long long mb = __ballot(before), me = __ballot(equal);
        if (WRITE) {
            const unsigned long long eq_front = run_e + (unsigned long long)__popcll(me & below);
            const unsigned long long r = run_b + (unsigned long long)__popcll(mb & below) + (eq_front < need ? eq_front : need);
            if ((before || (equal && eq_front < need)) && r < total) {
                if (ent) ent[r] = make_ulonglong2(w, d);
                else { ids[r] = d; reinterpret_cast<ulonglong2 *>(top)[r] = v; }
            }
        }
        run_b += (unsigned long long)__popcll(mb);
        run_e += (unsigned long long)__popcll(me);
    }
    if (!WRITE && lane == 0) { bsum[g] = run_b; esum[g] = run_e; }
}

// The sort.  A block's entry c of thread t is number 256 wave + 64 c + lane of the block: a wave walks its 256 in order.
__device__ __forceinline__ unsigned long long ts_index(int c) {
    return (unsigned long long)blockIdx.x * TS_BLOCK + (unsigned)((threadIdx.x >> 6) * (WAVE * TS_ITEMS) + c * WAVE + (threadIdx.x & (WAVE - 1)));
}
// the digit counts of each wave's 256 entries into cnt[wave][digit] (zeroed here; barriers in front and behind)
__device__ __forceinline__ void ts_count(const ulonglong2 (&e)[TS_ITEMS], unsigned long long n, int shift, unsigned *cnt) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) cnt[j * TOP_BINS + threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) {
        const bool have = ts_index(c) < n;
        const unsigned digit = (unsigned)(e[c].x >> shift) & (TOP_BINS - 1u);
        const unsigned long long m = wave_match_digit(digit, have);
        if (have && lane == __ffsll((long long)m) - 1)
            __hip_atomic_fetch_add(cnt + wave * TOP_BINS + digit, (unsigned)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
}
// Where entry c goes (n: it does not exist): the wave's base of its digit, which then moves on by the wave's entries
// with that digit -- the lanes in front of this one with the same digit come first.  Called by the whole wave, c ascending.
__device__ __forceinline__ unsigned long long ts_rank(const ulonglong2 e, bool have, unsigned long long n, int shift,
                                                      volatile unsigned long long *mine) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned digit = (unsigned)(e.x >> shift) & (TOP_BINS - 1u);
    const unsigned long long m = wave_match_digit(digit, have);
    const unsigned long long r = have ? mine[digit] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull)) : n;
    wave_lds_sync();                                                // every lane has its base before a leader moves it on
    if (have && lane == __ffsll((long long)m) - 1) mine[digit] += (unsigned long long)__popcll(m);
    wave_lds_sync();
    return r;
}
// the last pass's store: ids[r] = the id of rank r, top[r] = its pair (an id is one: nothing is read past the scores)
__device__ __forceinline__ void ts_store_last(unsigned long long r, unsigned long long id, unsigned long long *ids, pfac_doc_score *top,
                                              const pfac_doc_score *scores, unsigned long long n_docs) {
    if (id >= n_docs) return;
    ids[r] = id;
    reinterpret_cast<ulonglong2 *>(top)[r] = reinterpret_cast<const ulonglong2 *>(scores)[id];
}

// bh[digit * n_blocks + block] = the block's entries with that digit
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_top_sort_hist_kernel(const ulonglong2 *src, unsigned long long n, int shift, unsigned n_blocks, unsigned long long *bh) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    ulonglong2 e[TS_ITEMS];
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) e[c] = ts_index(c) < n ? src[ts_index(c)] : make_ulonglong2(0ull, 0ull);
    ts_count(e, n, shift, cnt);
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) sum += cnt[j * TOP_BINS + threadIdx.x];
    bh[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x] = sum;
}

// bh holds the exclusive prefixes.  dst != NULL: the entries move to dst; else (the last pass) the ids and the pairs.
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_top_sort_scatter_kernel(const ulonglong2 *src, unsigned long long n, int shift, unsigned n_blocks, const unsigned long long *bh,
                             ulonglong2 *dst, unsigned long long *ids, pfac_doc_score *top, const pfac_doc_score *scores,
                             unsigned long long n_docs) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    __shared__ unsigned long long base[TS_WAVES * TOP_BINS];
    ulonglong2 e[TS_ITEMS];
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) e[c] = ts_index(c) < n ? src[ts_index(c)] : make_ulonglong2(0ull, 0ull);
    ts_count(e, n, shift, cnt);
    unsigned long long acc = bh[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) { base[j * TOP_BINS + threadIdx.x] = acc; acc += cnt[j * TOP_BINS + threadIdx.x]; }
    __syncthreads();
    volatile unsigned long long *mine = base + (threadIdx.x >> 6) * TOP_BINS;     // this wave's bases: only its own lanes touch them
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) {
        const unsigned long long r = ts_rank(e[c], ts_index(c) < n, n, shift, mine);
        if (r < n) {
            if (dst) dst[r] = e[c];
            else ts_store_last(r, e[c].y, ids, top, scores, n_docs);
        }
    }
}

// n <= TS_BLOCK entries, ONE workgroup: every pass through LDS, the entries in registers in between.
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_top_sort_one_kernel(const ulonglong2 *src, unsigned long long n, unsigned long long *ids, pfac_doc_score *top,
                         const pfac_doc_score *scores, unsigned long long n_docs) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    __shared__ unsigned long long base[TS_WAVES * TOP_BINS];
    __shared__ ulonglong2 buf[TS_BLOCK];
    __shared__ unsigned wsum[TS_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    ulonglong2 e[TS_ITEMS];
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) e[c] = ts_index(c) < n ? src[ts_index(c)] : make_ulonglong2(0ull, 0ull);
    volatile unsigned long long *mine = base + wave * TOP_BINS;
    for (int pass = 0; pass < TOP_PASSES; pass++) {
        const int shift = pass * TOP_BITS;
        ts_count(e, n, shift, cnt);
        unsigned sum = 0;                                           // thread t: the entries with digit t, ...
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) sum += cnt[j * TOP_BINS + threadIdx.x];
        const unsigned incl = wave_incl_scan(sum);                  // ... and those with a smaller one: across the wave, then the waves
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        unsigned long long acc = incl - sum;
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) acc += j < wave ? wsum[j] : 0u;
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) { base[j * TOP_BINS + threadIdx.x] = acc; acc += cnt[j * TOP_BINS + threadIdx.x]; }
        __syncthreads();
        const bool last = pass == TOP_PASSES - 1;
#pragma unroll
        for (int c = 0; c < TS_ITEMS; c++) {
            const unsigned long long r = ts_rank(e[c], ts_index(c) < n, n, shift, mine);
            if (r < n) {
                if (last) ts_store_last(r, e[c].y, ids, top, scores, n_docs);
                else buf[r] = e[c];
            }
        }
        if (last) break;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TS_ITEMS; c++) e[c] = ts_index(c) < n ? buf[ts_index(c)] : make_ulonglong2(0ull, 0ull);
    }
}

// ---------------------------------------------------------------------------
// Term counts per document (pfac_documents_term_counts): the distinct (document, state) pairs of a record array that is
// already cut per document, with their multiplicities, as the three arrays of a CSR matrix.
//   pfac_tc_key_kernel       one lane per record, a wave per SS_RANGE records as in pfac_sel_scores_kernel: the record's
//                            document by the same bounded searches, key = doc << sbits | state (8 bytes, no payload),
//                            and the three checks (first[0] == 0, no decrease, every state below num_final) into one
//                            word.  Behind a failed check the keys are garbage in bounds and the host discards them.
//   the sort                 a stable LSD radix sort of the keys over the passes the host names (ceil of the key's bits
//                            / 8): siblings of the ranked sort's kernels over 8-byte entries, with the ballot ranks of
//                            ts_rank (wave_match_digit is shared, ts_count and ts_rank are not touched).  Per pass:
//                            pfac_tc_sort_hist_kernel (a workgroup takes `chunks` consecutive chunks of TC_BLOCK keys
//                            per histogram row: PFAC_TERMS_SORT_ROWS workgroups at most), pfac_tc_sort_rows_kernel (the
//                            prefix, one workgroup per digit over its row) and pfac_tc_sort_scatter_kernel.
//                            n <= TC_BLOCK: pfac_tc_sort_one_kernel, one workgroup, LDS.
//   pfac_tc_heads_kernel     entry i is a head iff i == 0 or key[i] != key[i - 1].  The compaction's shape: a wave per
//                            group of DM_BLOCKS blocks of 64 entries; kept per block: its 64-bit head ballot and the
//                            heads in front of it in its group; per group the sum, for pfac_scan_groups_kernel.
//   pfac_tc_write_kernel     behind the host's overflow check: the head of rank j stores states[j] = key & mask and its
//                            index into scratch, hidx[j] (hidx[n_terms] = n)
//   pfac_tc_counts_kernel    counts[j] = hidx[j + 1] - hidx[j]: no loop over a run of equal records
//   pfac_tc_rowptr_kernel    one lane per document: the sort keeps document d's records in [first[d], first[d + 1]), so
//                            row_ptr[d] = the heads in front of entry first[d] = group prefix + block prefix + a
//                            popcount of the block's ballot below that bit: no loop over a run of empty documents
constexpr int TC_BLOCK = TS_BLOCK;                                  // entries per chunk: wave w owns [256 w, 256 w + 256) of it
static_assert(TC_BLOCK == PFAC_TERMS_SORT_BLOCK, "the header names the sort's chunk size");
#define GRID_THREAD ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x)        // (as the document kernels define them)
#define GRID_THREADS ((unsigned long long)gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256)
pfac_tc_key_kernel(const pfac_record *sel, unsigned long long n, const unsigned long long *first, unsigned long long n_docs,
                   unsigned num_final, unsigned sbits, unsigned long long *keys, unsigned long long *bad_out) {
    bool bad = false;
    for (unsigned long long d = GRID_THREAD; d < n_docs; d += GRID_THREADS) bad = bad || first[d] > first[d + 1];
    if (GRID_THREAD == 0) bad = bad || first[0] != 0ull || first[n_docs] != n;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long p0 = ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SS_RANGE;
    if (p0 < n && n_docs) {                                     // (wave-uniform)
        const unsigned long long p1 = min(p0 + SS_RANGE, n);
        unsigned long long dlo = 0;
        for (unsigned long long c0 = p0; c0 < p1; c0 += WAVE) {
            const unsigned long long i = c0 + (unsigned)lane;
            const bool have = i < p1;
            dlo = doc_of(first, dlo, n_docs - 1, c0);
            const unsigned long long dhi = doc_of(first, dlo, n_docs - 1, min(c0 + (WAVE - 1), p1 - 1));
            const unsigned st = have ? sel[i].state : 0u;
            const bool known = st < num_final;
            bad = bad || !known;
            if (have) keys[i] = doc_of(first, dlo, dhi, i) << sbits | (known ? st : 0u);
        }
    }
    if (bad) bad_out[0] = 1ull;
}

// entry c of this thread in chunk `chunk`
__device__ __forceinline__ unsigned long long tc_index(unsigned long long chunk, int c) {
    return chunk * TC_BLOCK + (unsigned)((threadIdx.x >> 6) * (WAVE * TS_ITEMS) + c * WAVE + (threadIdx.x & (WAVE - 1)));
}
__device__ __forceinline__ void tc_load(unsigned long long (&e)[TS_ITEMS], const unsigned long long *src, unsigned long long chunk,
                                        unsigned long long n) {
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) e[c] = tc_index(chunk, c) < n ? src[tc_index(chunk, c)] : 0ull;
}
__device__ __forceinline__ void tc_zero(unsigned *cnt) {            // (barriers in front and behind)
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) cnt[j * TOP_BINS + threadIdx.x] = 0u;
    __syncthreads();
}
// ADDS the digit counts of each wave's 256 entries of the chunk to cnt[wave][digit] (no barrier: a wave's row is its own)
__device__ __forceinline__ void tc_count(const unsigned long long (&e)[TS_ITEMS], unsigned long long chunk, unsigned long long n,
                                         int shift, unsigned *cnt) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < TS_ITEMS; c++) {
        const bool have = tc_index(chunk, c) < n;
        const unsigned digit = (unsigned)(e[c] >> shift) & (TOP_BINS - 1u);
        const unsigned long long m = wave_match_digit(digit, have);
        if (have && lane == __ffsll((long long)m) - 1)
            __hip_atomic_fetch_add(cnt + wave * TOP_BINS + digit, (unsigned)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
// ts_rank over a key alone, with 32-bit bases (n < 2^32); the value of a lane without `have` means nothing
__device__ __forceinline__ unsigned tc_rank(unsigned long long e, bool have, int shift, volatile unsigned *mine) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned digit = (unsigned)(e >> shift) & (TOP_BINS - 1u);
    const unsigned long long m = wave_match_digit(digit, have);
    const unsigned r = have ? mine[digit] + (unsigned)__popcll(m & ((1ull << lane) - 1ull)) : 0u;
    wave_lds_sync();                                                // every lane has its base before a leader moves it on
    if (have && lane == __ffsll((long long)m) - 1) mine[digit] += (unsigned)__popcll(m);
    wave_lds_sync();
    return r;
}

// bh[digit * n_blocks + block] = the entries with that digit in the block's `chunks` chunks
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_tc_sort_hist_kernel(const unsigned long long *src, unsigned long long n, int shift, unsigned chunks, unsigned n_blocks,
                         unsigned *bh) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    tc_zero(cnt);
    for (unsigned ch = 0; ch < chunks; ch++) {
        const unsigned long long chunk = (unsigned long long)blockIdx.x * chunks + ch;
        if (chunk * TC_BLOCK >= n) break;
        unsigned long long e[TS_ITEMS];
        tc_load(e, src, chunk, n);
        tc_count(e, chunk, n, shift, cnt);
    }
    __syncthreads();
    unsigned sum = 0;
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) sum += cnt[j * TOP_BINS + threadIdx.x];
    bh[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x] = sum;
}

// The prefix of a pass, ONE WORKGROUP PER DIGIT: the digit's row of n_blocks counts becomes its exclusive prefix, in place,
// 256 counts per trip with the sum so far carried; tot[digit] = the row's sum.  (The ranked sort hands all 256 x n_blocks
// counts to the one workgroup of pfac_scan_groups_kernel: fine for its n_top, the whole pass here -- DESIGN.md, section 23.)
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_tc_sort_rows_kernel(unsigned *bh, unsigned n_blocks, unsigned *tot) {
    __shared__ unsigned wsum[TS_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    unsigned *row = bh + (unsigned long long)blockIdx.x * n_blocks;
    unsigned carry = 0;
    for (unsigned b0 = 0; b0 < n_blocks; b0 += TS_WAVES * WAVE) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned v = b < n_blocks ? row[b] : 0u;
        const unsigned incl = wave_incl_scan(v);
        __syncthreads();                                            // (the trip before has read wsum)
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        unsigned pre = carry + incl - v;
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) {
            pre += j < wave ? wsum[j] : 0u;
            carry += wsum[j];
        }
        if (b < n_blocks) row[b] = pre;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// bh holds the rows' exclusive prefixes, tot the rows' sums: digit t's first entry of this workgroup goes to the digits
// in front of t (a scan of tot, here) + the workgroups in front of this one with t.  Thread t keeps digit t's base in a
// register across the chunks, which go in order.
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_tc_sort_scatter_kernel(const unsigned long long *src, unsigned long long n, int shift, unsigned chunks, unsigned n_blocks,
                            const unsigned *bh, const unsigned *tot, unsigned long long *dst) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    __shared__ unsigned base[TS_WAVES * TOP_BINS];
    __shared__ unsigned wsum[TS_WAVES];
    const unsigned mytot = tot[threadIdx.x];
    const unsigned incl = wave_incl_scan(mytot);
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned run = incl - mytot + bh[(unsigned long long)threadIdx.x * n_blocks + blockIdx.x];
#pragma unroll
    for (int j = 0; j < TS_WAVES; j++) run += j < (int)(threadIdx.x >> 6) ? wsum[j] : 0u;
    volatile unsigned *mine = base + (threadIdx.x >> 6) * TOP_BINS;         // this wave's bases: only its own lanes touch them
    for (unsigned ch = 0; ch < chunks; ch++) {
        const unsigned long long chunk = (unsigned long long)blockIdx.x * chunks + ch;
        if (chunk * TC_BLOCK >= n) break;
        unsigned long long e[TS_ITEMS];
        tc_load(e, src, chunk, n);
        tc_zero(cnt);                                               // (its first barrier: every wave has left the chunk before)
        tc_count(e, chunk, n, shift, cnt);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) { base[j * TOP_BINS + threadIdx.x] = run; run += cnt[j * TOP_BINS + threadIdx.x]; }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TS_ITEMS; c++) {
            const bool have = tc_index(chunk, c) < n;
            const unsigned r = tc_rank(e[c], have, shift, mine);
            if (have && r < n) dst[r] = e[c];
        }
    }
}

// n <= TC_BLOCK keys, ONE workgroup, in place: every key is in a register before the first store.
__global__ void __launch_bounds__(TS_WAVES * WAVE)
pfac_tc_sort_one_kernel(unsigned long long *keys, unsigned long long n, int passes) {
    __shared__ unsigned cnt[TS_WAVES * TOP_BINS];
    __shared__ unsigned base[TS_WAVES * TOP_BINS];
    __shared__ unsigned long long buf[TC_BLOCK];
    __shared__ unsigned wsum[TS_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    unsigned long long e[TS_ITEMS];
    tc_load(e, keys, 0ull, n);
    volatile unsigned *mine = base + wave * TOP_BINS;
    for (int pass = 0; pass < passes; pass++) {
        const int shift = pass * TOP_BITS;
        tc_zero(cnt);
        tc_count(e, 0ull, n, shift, cnt);
        __syncthreads();
        unsigned sum = 0;                                           // thread t: the entries with digit t, ...
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) sum += cnt[j * TOP_BINS + threadIdx.x];
        const unsigned incl = wave_incl_scan(sum);                  // ... and those with a smaller one
        if (lane == WAVE - 1) wsum[wave] = incl;
        __syncthreads();
        unsigned acc = incl - sum;
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) acc += j < wave ? wsum[j] : 0u;
#pragma unroll
        for (int j = 0; j < TS_WAVES; j++) { base[j * TOP_BINS + threadIdx.x] = acc; acc += cnt[j * TOP_BINS + threadIdx.x]; }
        __syncthreads();
        const bool last = pass == passes - 1;
#pragma unroll
        for (int c = 0; c < TS_ITEMS; c++) {
            const bool have = tc_index(0ull, c) < n;
            const unsigned r = tc_rank(e[c], have, shift, mine);
            if (have && r < n) {
                if (last) keys[r] = e[c];
                else buf[r] = e[c];
            }
        }
        if (last) break;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TS_ITEMS; c++) e[c] = tc_index(0ull, c) < n ? buf[tc_index(0ull, c)] : 0ull;
    }
}

__global__ void __launch_bounds__(256)
pfac_tc_heads_kernel(const unsigned long long *keys, unsigned long long n, unsigned long long *bal, unsigned *X,
                     unsigned long long *gsum, unsigned n_groups) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long i0 = (unsigned long long)g * (DM_BLOCKS * WAVE);
    unsigned run = 0;
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long ib = i0 + (unsigned long long)b * WAVE, i = ib + lane;
        if (ib >= n) break;                                         // (wave-uniform)
        const bool have = i < n;
        const unsigned long long k = have ? keys[i] : 0ull;
        unsigned long long prev = __shfl_up(k, 1, WAVE);
        if (lane == 0 && i > 0) prev = keys[i - 1];
        const unsigned long long m = __ballot(have && (i == 0 || k != prev));
        if (lane == 0) { bal[ib >> 6] = m; X[ib >> 6] = run; }
        run += (unsigned)__popcll(m);
    }
    if (lane == 0) gsum[g] = run;
}

__global__ void __launch_bounds__(256)
pfac_tc_write_kernel(const unsigned long long *keys, unsigned long long n, const unsigned long long *bal, const unsigned *X,
                     const unsigned long long *gpre, unsigned n_groups, unsigned long long mask, unsigned long long n_terms,
                     unsigned *states, unsigned *hidx) {
    if (GRID_THREAD == 0) hidx[n_terms] = (unsigned)n;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long i0 = (unsigned long long)g * (DM_BLOCKS * WAVE), pre = gpre[g];
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long ib = i0 + (unsigned long long)b * WAVE, i = ib + lane;
        if (ib >= n) break;
        const unsigned long long m = bal[ib >> 6];
        const unsigned long long j = pre + X[ib >> 6] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && i < n && j < n_terms) {
            states[j] = (unsigned)(keys[i] & mask);
            hidx[j] = (unsigned)i;
        }
    }
}

__global__ void __launch_bounds__(256)
pfac_tc_counts_kernel(const unsigned *hidx, unsigned long long n_terms, unsigned *counts) {
    for (unsigned long long j = GRID_THREAD; j < n_terms; j += GRID_THREADS) counts[j] = hidx[j + 1] - hidx[j];
}

__global__ void __launch_bounds__(256)
pfac_tc_rowptr_kernel(const unsigned long long *first, unsigned long long n_docs, unsigned long long n, const unsigned long long *bal,
                      const unsigned *X, const unsigned long long *gpre, unsigned long long n_terms, unsigned long long *row) {
    for (unsigned long long d = GRID_THREAD; d <= n_docs; d += GRID_THREADS) {
        const unsigned long long i = first[d];
        row[d] = i >= n ? n_terms
                        : gpre[i / (DM_BLOCKS * WAVE)] + X[i >> 6] + (unsigned long long)__popcll(bal[i >> 6] & ((1ull << (i & 63)) - 1ull));
    }
}

// ---------------------------------------------------------------------------
// Rule sets (pfac_documents_rules): the join of a document-term matrix (row_ptr, states) with the state-major rule table
// of pfac_table_set_rules (sptr[num_final + 1], ent[] = rule << 1 | negated, need[n_rules]).  A pair is one (document,
// state) of the matrix; pair i expands into c_i = sptr[s + 1] - sptr[s] keys, E keys in all.
//   pfac_ru_count_kernel     a wave per group of DM_BLOCKS blocks of 64 pairs: the pair's document by the bounded searches
//                            of pfac_tc_key_kernel, c_i, and the four checks (row_ptr[0] == 0, no decrease, every state
//                            below num_final, the states strictly ascending inside a row) into one word.  Kept per pair:
//                            its document and the keys in front of it in its group (32 bits: they mean something only
//                            while E < 2^32, which the host checks); per group the 64-bit sum, for pfac_scan_groups_kernel.
//   pfac_ru_expand_kernel    output-driven, one lane per key e < E: its group by a search in the group prefixes, its pair
//                            by a search in the group's 4096 pair prefixes, its entry at sptr[s] + (e - the pair's first
//                            key): key[e] = doc << (rbits + 1) | rule << 1 | negated.  No loop is as long as a state's
//                            rule count.
//   the sort                 tc_sort: the term counts' kernels over ceil((dbits + rbits + 1) / 8) digits
//   pfac_ru_fired_kernel     a (document, rule) run is contiguous now, positive entries first, every entry another term.
//                            Entry t is a tail iff t == E - 1 or key[t + 1] >> 1 != key[t] >> 1; the run fires iff the tail
//                            is positive (no negated term present) and key[t - (need - 1)] is of the same run (need
//                            positive terms present).  The compaction's shape, as pfac_tc_heads_kernel.
//   pfac_ru_write_kernel     behind the host's overflow check: the fired tail of rank j stores rules[j]
//   pfac_ru_rowptr_kernel    one lane per document: the lower bound of d << (rbits + 1) in the sorted keys is the
//                            document's first entry; the fired tails in front of it are two loads and a popcount
__global__ void __launch_bounds__(256)
pfac_ru_count_kernel(const unsigned long long *row, unsigned long long n_docs, const unsigned *states, unsigned long long n,
                     const unsigned *sptr, unsigned num_final, unsigned *cpre, unsigned *pdoc, unsigned long long *gsum,
                     unsigned n_groups, unsigned long long *bad_out) {
    bool bad = false;
    for (unsigned long long d = GRID_THREAD; d < n_docs; d += GRID_THREADS) bad = bad || row[d] > row[d + 1];
    if (GRID_THREAD == 0) bad = bad || row[0] != 0ull || row[n_docs] != n;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g < n_groups && n_docs) {                               // (wave-uniform)
        const unsigned long long p0 = (unsigned long long)g * (DM_BLOCKS * WAVE), p1 = min(p0 + DM_BLOCKS * WAVE, n);
        unsigned long long dlo = 0, run = 0;
        for (unsigned long long c0 = p0; c0 < p1; c0 += WAVE) {
            const unsigned long long i = c0 + (unsigned)lane;
            const bool have = i < p1;
            dlo = doc_of(row, dlo, n_docs - 1, c0);
            const unsigned long long dhi = doc_of(row, dlo, n_docs - 1, min(c0 + (WAVE - 1), p1 - 1));
            const unsigned long long d = have ? doc_of(row, dlo, dhi, i) : dlo;
            const unsigned st = have ? states[i] : 0u;
            const bool known = st < num_final;
            unsigned prev = (unsigned)__shfl_up((int)st, 1, WAVE);
            if (lane == 0 && c0 > 0) prev = states[c0 - 1];
            bad = bad || (have && (!known || (i > row[d] && prev >= st)));
            const unsigned c = have && known ? sptr[st + 1] - sptr[st] : 0u;
            const unsigned incl = wave_incl_scan(c);
            if (have) { cpre[i] = (unsigned)run + incl - c; pdoc[i] = (unsigned)d; }
            run += wave_sum64(c);
        }
        if (lane == 0) gsum[g] = run;
    }
    if (bad) bad_out[0] = 1ull;
}

__global__ void __launch_bounds__(256)
pfac_ru_expand_kernel(const unsigned *states, unsigned long long n, const unsigned *cpre, const unsigned *pdoc,
                      const unsigned long long *gpre, unsigned n_groups, const unsigned *sptr, const unsigned *ent,
                      unsigned rbits, unsigned long long n_keys, unsigned long long *keys) {
    for (unsigned long long e = GRID_THREAD; e < n_keys; e += GRID_THREADS) {
        unsigned glo = 0, ghi = n_groups - 1;                   // the last group with gpre[g] <= e
        while (glo < ghi) {
            const unsigned mid = (glo + ghi + 1) >> 1;
            if (gpre[mid] <= e) glo = mid;
            else ghi = mid - 1;
        }
        const unsigned x = (unsigned)(e - gpre[glo]);
        unsigned long long lo = (unsigned long long)glo * (DM_BLOCKS * WAVE), hi = min(lo + DM_BLOCKS * WAVE, n) - 1;
        while (lo < hi) {                                       // the last pair of the group with cpre[i] <= x
            const unsigned long long mid = (lo + hi + 1) >> 1;
            if (cpre[mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        const unsigned entry = ent[sptr[states[lo]] + (x - cpre[lo])];
        keys[e] = (unsigned long long)pdoc[lo] << (rbits + 1u) | entry;
    }
}

__global__ void __launch_bounds__(256)
pfac_ru_fired_kernel(const unsigned long long *keys, unsigned long long n, const unsigned *need, unsigned rmask,
                     unsigned long long *bal, unsigned *X, unsigned long long *gsum, unsigned n_groups) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long i0 = (unsigned long long)g * (DM_BLOCKS * WAVE);
    unsigned run = 0;
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long ib = i0 + (unsigned long long)b * WAVE, i = ib + lane;
        if (ib >= n) break;                                         // (wave-uniform)
        const bool have = i < n;
        const unsigned long long k = have ? keys[i] : 0ull;
        unsigned long long next = __shfl_down(k, 1, WAVE);
        if (lane == WAVE - 1 && i + 1 < n) next = keys[i + 1];
        bool fires = have && !(k & 1ull) && (i + 1 == n || (next >> 1) != (k >> 1));
        if (fires) {
            const unsigned back = need[(unsigned)(k >> 1) & rmask] - 1u;
            fires = i >= back && (keys[i - back] >> 1) == (k >> 1);
        }
        const unsigned long long m = __ballot(fires);
        if (lane == 0) { bal[ib >> 6] = m; X[ib >> 6] = run; }
        run += (unsigned)__popcll(m);
    }
    if (lane == 0) gsum[g] = run;
}

__global__ void __launch_bounds__(256)
pfac_ru_write_kernel(const unsigned long long *keys, unsigned long long n, const unsigned long long *bal, const unsigned *X,
                     const unsigned long long *gpre, unsigned n_groups, unsigned rmask, unsigned long long n_fired,
                     unsigned *rules) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const unsigned long long i0 = (unsigned long long)g * (DM_BLOCKS * WAVE), pre = gpre[g];
    for (int b = 0; b < DM_BLOCKS; b++) {
        const unsigned long long ib = i0 + (unsigned long long)b * WAVE, i = ib + lane;
        if (ib >= n) break;
        const unsigned long long m = bal[ib >> 6];
        const unsigned long long j = pre + X[ib >> 6] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && i < n && j < n_fired) rules[j] = (unsigned)(keys[i] >> 1) & rmask;
    }
}

__global__ void __launch_bounds__(256)
pfac_ru_rowptr_kernel(const unsigned long long *keys, unsigned long long n, unsigned long long n_docs, unsigned rbits,
                      const unsigned long long *bal, const unsigned *X, const unsigned long long *gpre,
                      unsigned long long n_fired, unsigned long long *row) {
    for (unsigned long long d = GRID_THREAD; d <= n_docs; d += GRID_THREADS) {
        unsigned long long i = n;
        if (d < n_docs) i = doc_lower_bound(keys, n, d << (rbits + 1u));
        row[d] = i >= n ? n_fired
                        : gpre[i / (DM_BLOCKS * WAVE)] + X[i >> 6] + (unsigned long long)__popcll(bal[i >> 6] & ((1ull << (i & 63)) - 1ull));
    }
}
#undef GRID_THREAD
#undef GRID_THREADS

// ---------------------------------------------------------------------------
// The selected documents' bytes, back to back (pfac_documents_gather): segment k is in[off[ids[k]], off[ids[k] + 1]), at
// output offset out_off[k] = the sum of the lengths before it.  The replace's shape with the picks taken out:
//   pfac_ga_count_kernel     one workgroup per 1024 ids: two 8-byte gathers of the offsets per id, the checks (id <
//                            n_docs, off[id] <= off[id + 1] <= n_bytes) into an error word, per block of 64 ids X[b] = the
//                            lengths before it in its group, and the group's sum
//   pfac_scan_groups_kernel  the group prefixes and the total = out_bytes, which the host checks before anything is written
//   pfac_ga_offsets_kernel   one wave per block: out_off[k] for every id, out_off[n_ids] = out_bytes
//   pfac_ga_write_kernel     output-driven, the replace's loop (rp_write_windows) -- never a walk from id 0, and blocks
//                            of empty documents are skipped -- over its own block: 65 output offsets and 64 source
//                            offsets in LDS, and a segment that is one piece, an unaligned source run (rp_merge).
// A block's prefix is O_{64b} = X[b] + gpre[b / RP_GROUP] (rp_block_out), as in the replace.

__global__ void __launch_bounds__(RP_GROUP / 4 * WAVE)
pfac_ga_count_kernel(const unsigned long long *ids, unsigned long long n, const unsigned long long *off, unsigned long long n_docs,
                     unsigned long long n_bytes, unsigned long long *X, unsigned long long *gsum, unsigned long long *res) {
    __shared__ unsigned long long bsum[RP_GROUP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = (n + RP_BLOCK - 1) / RP_BLOCK;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned lb = (unsigned)w * 4 + (unsigned)i;
        const unsigned long long k = ((unsigned long long)blockIdx.x * RP_GROUP + lb) * RP_BLOCK + (unsigned)lane;
        unsigned long long len = 0;
        if (k < n) {
            const unsigned long long id = ids[k];
            if (id < n_docs) {
                const unsigned long long lo = off[id], hi = off[id + 1];
                if (lo <= hi && hi <= n_bytes) len = hi - lo;
                else bad = true;
            } else {
                bad = true;
            }
        }
        const unsigned long long s = wave_sum64(len);
        if (lane == 0) bsum[lb] = s;
    }
    if (__ballot(bad) && lane == 0) atomicOr(&res[0], 1ull);
    rp_count_out(bsum, nb, X, gsum, [](unsigned) { return 0ull; });
}

// (behind the host's check of the count pass: every id is below n_docs and its offsets ascend)
__global__ void __launch_bounds__(4 * WAVE)
pfac_ga_offsets_kernel(const unsigned long long *ids, unsigned long long n, const unsigned long long *off,
                       const unsigned long long *X, const unsigned long long *gpre, unsigned long long *out_off) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long b = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6), k = b * RP_BLOCK + (unsigned)lane;
    if (b * RP_BLOCK >= n) return;
    unsigned long long len = 0;
    if (k < n) {
        const unsigned long long id = ids[k];
        len = off[id + 1] - off[id];
    }
    rp_block_offsets(rp_block_out(X, gpre, b), len, k, n, out_off);
}

__global__ void __launch_bounds__(RP_WAVES * WAVE)
pfac_ga_write_kernel(const unsigned char *in, unsigned long long n_bytes, const unsigned long long *ids, unsigned long long n,
                     const unsigned long long *off, const unsigned long long *out_off, const unsigned long long *X,
                     const unsigned long long *gpre, unsigned long long out_bytes, unsigned wins, unsigned char *out) {
    __shared__ unsigned long long s_o[RP_WAVES][RP_BLOCK + 1];      // segment k's output offset (k = cnt: the block's end)
    __shared__ unsigned long long s_src[RP_WAVES][RP_BLOCK];        // where it starts in the input
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = (n + RP_BLOCK - 1) / RP_BLOCK;    // (n > 0: there are output bytes)
    unsigned long long *so = s_o[w], *ssrc = s_src[w];
    auto load_block = [&](unsigned long long b, unsigned long long &Ob, unsigned long long &hi, unsigned &cnt) {
        const unsigned long long k = b * RP_BLOCK + (unsigned)lane;
        cnt = (unsigned)min((unsigned long long)RP_BLOCK, n - b * RP_BLOCK);
        if (k <= n) so[lane] = out_off[k];                          // (lane <= cnt; out_off has n + 1 entries)
        if (k < n) ssrc[lane] = off[ids[k]];
        if (lane == 0 && cnt == (unsigned)RP_BLOCK) so[RP_BLOCK] = out_off[k + RP_BLOCK];
        wave_lds_sync();
        Ob = so[0];
        hi = so[cnt];
    };
    rp_write_windows(lane, w, X, gpre, nb, out_bytes, wins, out, load_block,
                     [&](unsigned cnt, uint4 &acc, unsigned long long o, unsigned long long pos, unsigned long long e) {
        const unsigned l = rp_segment(so, cnt, pos);                // (k < cnt: so[k + 1] > pos)
        const unsigned long long pe = min(so[l + 1], e);
        rp_merge(acc, in, (long long)(ssrc[l] + o - so[l]), n_bytes, (unsigned)(pos - o), (unsigned)(pe - o));
        return pe;
    });
}

// ---------------------------------------------------------------------------
// The gather with labels (pfac_documents_gather_format: grep -n, -b, the "--" lines of -A / -B / -C, the final
// newline).  Segment k is up to five pieces: the group separator (ids[k] does not follow ids[k - 1]), the decimal of
// the line number and its label separator, the decimal of the byte offset and its label separator, the body, and the
// terminator where the body lacks it.  The gather's shape, as siblings of its kernels (the plain gather's are not
// touched: they keep their code):
//   pfac_gf_count_kernel     the gather's count with gf_segment_len for the length: besides the two offset gathers the
//                            id in front (a lane shuffle; a load for lane 0) and, under TERMINATE, the body's last byte
//   pfac_scan_groups_kernel
//   pfac_gf_offsets_kernel   out_off[k] from the same lengths
//   pfac_gf_write_kernel     rp_write_windows over a block whose LDS also holds each segment's id, its source offset
//                            and, in one 32-bit word, its piece lengths.  The digits a lane owns are made in registers:
//                            one divide by a power of ten, then peeled by 10.  No scratch copy of the labels, no second
//                            pass over the output.

struct GfFormat {
    unsigned flags;                         // PFAC_LINE_*
    unsigned sep_len;                       // group_sep_len
    unsigned chars;                         // sep_match | sep_context << 8 | terminator << 16
    unsigned long long sep;                 // group_sep, byte i at bits [8 i, 8 i + 8)
    unsigned long long number_base, offset_base;
};

// piece lengths of a segment in one word: the group separator (0..8), the number with its label separator (0..19), the
// offset with its (0..19), the terminator (0..1), and whether the label separator is sep_context
constexpr unsigned GF_NUM_SHIFT = 4, GF_OFF_SHIFT = 9, GF_TERM_SHIFT = 14, GF_CTX_SHIFT = 15;

// the pieces in front of the body of the segment of document id at source offset lo, `follows`: id == the id in front + 1
__device__ __forceinline__ unsigned gf_head_pieces(const GfFormat &f, unsigned long long id, unsigned long long lo, bool first,
                                                   bool follows) {
    unsigned w = 0;
    if (first ? (f.flags & PFAC_LINE_SEP_FIRST) != 0 : !follows) w = f.sep_len;
    if (f.flags & PFAC_LINE_NUMBER) w |= (ndigits64(id + f.number_base) + 1u) << GF_NUM_SHIFT;
    if (f.flags & PFAC_LINE_OFFSET) w |= (ndigits64(lo + f.offset_base) + 1u) << GF_OFF_SHIFT;
    return w;
}
__device__ __forceinline__ unsigned gf_head_len(unsigned w) {
    return (w & 15u) + ((w >> GF_NUM_SHIFT) & 31u) + ((w >> GF_OFF_SHIFT) & 31u);
}

// Length of segment k (valid id, lo <= hi <= n_bytes): lane `lane` of a wave whose lanes hold consecutive k
__device__ __forceinline__ unsigned long long gf_segment_len(const GfFormat &f, const unsigned char *in, const unsigned long long *ids,
                                                             unsigned long long k, unsigned long long id, bool ok,
                                                             unsigned long long lo, unsigned long long hi, int lane) {
    unsigned long long prev = __shfl_up(id, 1u, WAVE);
    if (lane == 0 && k > 0 && ok) prev = ids[k - 1];
    if (!ok) return 0ull;
    unsigned long long len = gf_head_len(gf_head_pieces(f, id, lo, k == 0, id == prev + 1)) + (hi - lo);
    if (f.flags & PFAC_LINE_TERMINATE) len += (hi == lo || in[hi - 1] != (unsigned char)(f.chars >> 16)) ? 1u : 0u;
    return len;
}

__global__ void __launch_bounds__(RP_GROUP / 4 * WAVE)
pfac_gf_count_kernel(const unsigned char *in, const unsigned long long *ids, unsigned long long n, const unsigned long long *off,
                     unsigned long long n_docs, unsigned long long n_bytes, GfFormat f, unsigned long long *X,
                     unsigned long long *gsum, unsigned long long *res) {
    __shared__ unsigned long long bsum[RP_GROUP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = (n + RP_BLOCK - 1) / RP_BLOCK;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned lb = (unsigned)w * 4 + (unsigned)i;
        const unsigned long long k = ((unsigned long long)blockIdx.x * RP_GROUP + lb) * RP_BLOCK + (unsigned)lane;
        unsigned long long id = 0, lo = 0, hi = 0;
        bool ok = false;
        if (k < n) {
            id = ids[k];
            if (id < n_docs) {
                lo = off[id];
                hi = off[id + 1];
                ok = lo <= hi && hi <= n_bytes;
            }
            bad |= !ok;
        }
        const unsigned long long s = wave_sum64(gf_segment_len(f, in, ids, k, id, ok, lo, hi, lane));
        if (lane == 0) bsum[lb] = s;
    }
    if (__ballot(bad) && lane == 0) atomicOr(&res[0], 1ull);
    rp_count_out(bsum, nb, X, gsum, [](unsigned) { return 0ull; });
}

// (behind the host's check of the count pass: every id is below n_docs and its offsets ascend)
__global__ void __launch_bounds__(4 * WAVE)
pfac_gf_offsets_kernel(const unsigned char *in, const unsigned long long *ids, unsigned long long n, const unsigned long long *off,
                       GfFormat f, const unsigned long long *X, const unsigned long long *gpre, unsigned long long *out_off) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long b = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6), k = b * RP_BLOCK + (unsigned)lane;
    if (b * RP_BLOCK >= n) return;
    unsigned long long id = 0, lo = 0, hi = 0;
    if (k < n) {
        id = ids[k];
        lo = off[id];
        hi = off[id + 1];
    }
    rp_block_offsets(rp_block_out(X, gpre, b), gf_segment_len(f, in, ids, k, id, k < n, lo, hi, lane), k, n, out_off);
}

// acc bytes [j0, j1) := bytes [j0, j1) of the 16 bytes (hi : lo), lo's lowest byte being byte 0
__device__ __forceinline__ void gf_put(uint4 &acc, unsigned long long lo, unsigned long long hi, unsigned j0, unsigned j1) {
    auto low = [](int m) -> unsigned { return m <= 0 ? 0u : m >= 4 ? 0xffffffffu : (1u << (8 * m)) - 1u; };
    const unsigned m0 = low((int)j1) & ~low((int)j0), m1 = low((int)j1 - 4) & ~low((int)j0 - 4);
    const unsigned m2 = low((int)j1 - 8) & ~low((int)j0 - 8), m3 = low((int)j1 - 12) & ~low((int)j0 - 12);
    acc.x = (acc.x & ~m0) | ((unsigned)lo & m0);
    acc.y = (acc.y & ~m1) | ((unsigned)(lo >> 32) & m1);
    acc.z = (acc.z & ~m2) | ((unsigned)hi & m2);
    acc.w = (acc.w & ~m3) | ((unsigned)(hi >> 32) & m3);
}
// byte c at byte j (0..15) of (hi : lo)
__device__ __forceinline__ void gf_byte(unsigned long long &lo, unsigned long long &hi, unsigned j, unsigned c) {
    if (j < 8u) lo |= (unsigned long long)c << (8u * j);
    else hi |= (unsigned long long)c << (8u * (j - 8u));
}

__device__ __forceinline__ unsigned long long gf_pow10(unsigned e) {         // e <= 17
    unsigned long long p = e & 1u ? 10ull : 1ull;
    if (e & 2u) p *= 100ull;
    if (e & 4u) p *= 10000ull;
    if (e & 8u) p *= 100000000ull;
    if (e & 16u) p *= 10000000000000000ull;
    return p;
}

// 16 bytes in registers that grow at the front: push(c) makes c byte 0 and moves the others up by one
struct GfBytes {
    unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    __device__ __forceinline__ void push(unsigned c) {
        w3 = __builtin_amdgcn_alignbit(w3, w2, 24);
        w2 = __builtin_amdgcn_alignbit(w2, w1, 24);
        w1 = __builtin_amdgcn_alignbit(w1, w0, 24);
        w0 = w0 << 8 | c;
    }
    // acc bytes [j0, j1) := bytes [0, j1 - j0)
    __device__ __forceinline__ void put(uint4 &acc, unsigned j0, unsigned j1) const {
        const unsigned q = j0 >> 2, r = 8u * (j0 & 3u);
        const unsigned y0 = q == 0 ? w0 : 0u, y1 = q == 0 ? w1 : q == 1 ? w0 : 0u;
        const unsigned y2 = q == 0 ? w2 : q == 1 ? w1 : q == 2 ? w0 : 0u, y3 = q == 0 ? w3 : q == 1 ? w2 : q == 2 ? w1 : w0;
        const unsigned long long lo = (unsigned long long)y1 << 32 | y0, hi = (unsigned long long)y3 << 32 | y2;
        gf_put(acc, lo << r, r ? hi << r | lo >> (64u - r) : hi, j0, j1);
    }
};

// The bytes [pos, pe) of a label -- the nd digits of v, then the label separator c -- that starts at output offset ps,
// into the chunk at o (pos >= o, pe <= o + 16, pe <= ps + nd + 1): digits [pos - ps, min(pe - ps, nd)) of v, the most
// significant being digit 0, by one divide (only where the chunk ends inside the digits) and a peel from the least
// significant of them, in 32 bits as soon as the value fits.
__device__ __forceinline__ void gf_label(uint4 &acc, unsigned long long o, unsigned long long ps, unsigned nd, unsigned long long v,
                                         unsigned c, unsigned long long pos, unsigned long long pe) {
    GfBytes w;
    const unsigned d0 = (unsigned)(pos - ps);
    unsigned d1 = (unsigned)(pe - ps);
    if (d1 > nd) {
        w.push(c);
        d1 = nd;
    }
    if (d1 > d0) {
        unsigned cnt = d1 - d0;
        if (v >> 32) {
            if (d1 < nd) v /= gf_pow10(nd - d1);
            while (cnt && (v >> 32)) {
                const unsigned long long q = v / 10ull;
                w.push((unsigned)'0' + (unsigned)(v - q * 10ull));
                v = q;
                cnt--;
            }
        } else if (d1 < nd) {
            v = (unsigned)v / (unsigned)gf_pow10(nd - d1);
        }
        unsigned v32 = (unsigned)v;
        while (cnt) {
            const unsigned q = v32 / 10u;
            w.push((unsigned)'0' + (v32 - q * 10u));
            v32 = q;
            cnt--;
        }
    }
    w.put(acc, (unsigned)(pos - o), (unsigned)(pe - o));
}

__global__ void __launch_bounds__(RP_WAVES * WAVE)
pfac_gf_write_kernel(const unsigned char *in, unsigned long long n_bytes, const unsigned long long *ids, unsigned long long n,
                     const unsigned long long *off, const unsigned long long *doc_first, GfFormat f,
                     const unsigned long long *out_off, const unsigned long long *X, const unsigned long long *gpre,
                     unsigned long long out_bytes, unsigned wins, unsigned char *out) {
    __shared__ unsigned long long s_o[RP_WAVES][RP_BLOCK + 1];      // segment k's output offset (k = cnt: the block's end)
    __shared__ unsigned long long s_src[RP_WAVES][RP_BLOCK];        // where its body starts in the input
    __shared__ unsigned s_id[RP_WAVES][RP_BLOCK];                   // its document (below 2^32)
    __shared__ unsigned s_pc[RP_WAVES][RP_BLOCK];                   // its piece lengths
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned long long nb = (n + RP_BLOCK - 1) / RP_BLOCK;    // (n > 0: there are output bytes)
    unsigned long long *so = s_o[w], *ssrc = s_src[w];
    unsigned *sid = s_id[w], *spc = s_pc[w];
    auto load_block = [&](unsigned long long b, unsigned long long &Ob, unsigned long long &hi, unsigned &cnt) {
        const unsigned long long k = b * RP_BLOCK + (unsigned)lane;
        cnt = (unsigned)min((unsigned long long)RP_BLOCK, n - b * RP_BLOCK);
        unsigned long long id = 0;
        if (k < n) id = ids[k];
        unsigned long long prev = __shfl_up(id, 1u, WAVE);
        if (lane == 0 && k > 0) prev = ids[k - 1];
        if (k <= n) so[lane] = out_off[k];                          // (lane <= cnt; out_off has n + 1 entries)
        if (k < n) {
            const unsigned long long lo = off[id], len = out_off[k + 1] - out_off[k];
            unsigned pc = gf_head_pieces(f, id, lo, k == 0, id == prev + 1);
            // (the terminator is what the count pass added to the head and the body)
            pc |= (unsigned)(len - gf_head_len(pc) - (off[id + 1] - lo)) << GF_TERM_SHIFT;
            if ((f.flags & PFAC_LINE_CONTEXT_SEP) && doc_first[id + 1] == doc_first[id]) pc |= 1u << GF_CTX_SHIFT;
            ssrc[lane] = lo;
            sid[lane] = (unsigned)id;
            spc[lane] = pc;
        }
        if (lane == 0 && cnt == (unsigned)RP_BLOCK) so[RP_BLOCK] = out_off[k + RP_BLOCK];
        wave_lds_sync();
        Ob = so[0];
        hi = so[cnt];
    };
    rp_write_windows(lane, w, X, gpre, nb, out_bytes, wins, out, load_block,
                     [&](unsigned cnt, uint4 &acc, unsigned long long o, unsigned long long pos, unsigned long long e) {
        // everything of the segment that holds pos inside [pos, e), in one call: the bisection runs once per segment
        // and chunk, as in the plain gather, however many pieces the segment has
        const unsigned l = rp_segment(so, cnt, pos);                // (k < cnt: so[k + 1] > pos)
        const unsigned pc = spc[l];
        const unsigned long long end = so[l + 1], pe = min(end, e);
        unsigned long long ps = so[l], pn = ps + (pc & 15u);        // the piece at hand is [ps, pn); [a, b) of it lies in [pos, pe)
        unsigned long long a = max(ps, pos), b = min(pn, pe);
        if (a < b) {                                                // the group separator
            const long long sh = (long long)(ps - o);               // -8 < sh < 16
            const unsigned long long lo = sh < 0 ? f.sep >> (unsigned)(-8 * sh) : sh < 8 ? f.sep << (unsigned)(8 * sh) : 0ull;
            const unsigned long long hi = sh <= 0 ? 0ull : sh < 8 ? f.sep >> (unsigned)(64 - 8 * sh) : f.sep << (unsigned)(8 * (sh - 8));
            gf_put(acc, lo, hi, (unsigned)(a - o), (unsigned)(b - o));
        }
        const unsigned c = pc >> GF_CTX_SHIFT & 1u ? f.chars >> 8 & 255u : f.chars & 255u;
        ps = pn;
        pn = ps + ((pc >> GF_NUM_SHIFT) & 31u);
        a = max(ps, pos);
        b = min(pn, pe);
        if (a < b)                                                  // the line number
            gf_label(acc, o, ps, (unsigned)(pn - ps) - 1u, (unsigned long long)sid[l] + f.number_base, c, a, b);
        ps = pn;
        pn = ps + ((pc >> GF_OFF_SHIFT) & 31u);
        a = max(ps, pos);
        b = min(pn, pe);
        if (a < b)                                                  // the byte offset
            gf_label(acc, o, ps, (unsigned)(pn - ps) - 1u, ssrc[l] + f.offset_base, c, a, b);
        ps = pn;
        pn = end - ((pc >> GF_TERM_SHIFT) & 1u);
        a = max(ps, pos);
        b = min(pn, pe);
        if (a < b)                                                  // the body
            rp_merge(acc, in, (long long)(ssrc[l] + o - ps), n_bytes, (unsigned)(a - o), (unsigned)(b - o));
        if (pn < end && pe == end) {                                // the terminator: the segment's last byte (end - 1 >= pos)
            unsigned long long lo = 0, hi = 0;
            gf_byte(lo, hi, (unsigned)(pn - o), f.chars >> 16 & 255u);
            gf_put(acc, lo, hi, (unsigned)(pn - o), (unsigned)(pn - o) + 1u);
        }
        return pe;
    });
}

// ---------------------------------------------------------------------------
// Token ids of the leftmost-longest picks (pfac_tokenize_leftmost_longest, pfac_tokenize_documents).  Position i of
// [entry, n_owned) emits tok[s_k] at a pick's start, btok[input[i]] outside every pick, nothing inside one; DROP emits
// nothing.  The number of tokens in a gap depends on the gap's bytes and a gap has no length bound, so the pass is
// position-driven, over the scan's 4 KiB tiles, not pick-driven like the replace:
//   pfac_tk_first_kernel     one thread per tile: first[t] = the first pick at or behind the tile's start (a lower bound
//                            over sel[].pos), first[n_tiles] = n.  Patterns are shorter than HALO_MAX, so the one pick
//                            that can reach into tile t from the front is pick first[t] - 1.
//   pfac_tk_count_kernel     a workgroup per group of 64 tiles, a wave per tile at a time.  The lanes that own the tile's
//                            picks set the coverage bits (and the start bit where tok[s] != DROP) in LDS, the byte lanes
//                            look their 16 bytes up in btok (LDS); emits = (byte & ~covered | start) & [entry, n_owned).
//                            Kept per tile: the 64 bitmap words, the 16-bit count of the tokens in front of each word,
//                            and the tokens in front of the tile in its group; per group the sum.  Every pick is checked
//                            by the one tile that owns its start (state, length, inside the tile and below n_owned, not
//                            before the end of the pick in front of it), and first[] must not decrease: with first[0]
//                            == 0 and first[n_tiles] == n that covers every pick exactly once.
//   pfac_scan_groups_kernel  the group prefixes and the total, which the host checks before anything is written
//   pfac_tk_write_kernel     one wave per tile.  The tile's tokens are ids[base .. base + cnt), base = group prefix +
//                            tile prefix.  A token's rank is its word's prefix + a popcount of the saved bitmap below its
//                            bit; the values are staged in LDS in rank order, shifted by base & 3 so that LDS chunk c is
//                            the aligned 16 bytes of the output, and stored as whole dwordx4 where all four entries are
//                            the tile's, in pieces at the two ragged ends.  Byte tokens are staged first, then the pick
//                            tokens over them (a kept pick start is the one emitting position whose byte is not its
//                            value).  A lane whose 16 positions emit nothing loads no input.
//   pfac_tk_doc_kernel       one thread per document: tok_off[d] = group prefix + tile prefix + word prefix + a popcount
//                            of the word below off[d]; off[d] == n_owned gives the total.
constexpr int TK_GROUP = 64;                        // tiles per workgroup of the count kernel (one group of the prefix)
constexpr int TK_WAVES = 4;                         // its waves: 16 tiles each
constexpr int TK_WORDS = WTILE / 64;                // bitmap words of a tile
constexpr int TK_STAGE = WTILE + 4;                 // staged entries of the write: a full tile shifted by up to 3
static_assert(TK_WORDS == WAVE, "a lane per bitmap word");

__device__ __forceinline__ unsigned long long tk_below(unsigned bit) { return (1ull << bit) - 1ull; }   // bit < 64

__global__ void pfac_tk_first_kernel(const pfac_record *sel, unsigned long long n, unsigned long long n_tiles,
                                     unsigned long long *first) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    unsigned long long lo = 0, hi = n;
    if (t == n_tiles) lo = n;
    const unsigned long long start = t * WTILE;
    while (lo < hi) {
        const unsigned long long m = lo + (hi - lo) / 2;
        if ((unsigned long long)sel[m].pos < start) lo = m + 1;
        else hi = m;
    }
    first[t] = lo;
}

// 16 input bytes at the 16-aligned position g; bytes at or past n_avail read as 0
__device__ __forceinline__ uint4 tk_load16(const unsigned char *in, unsigned long long g, unsigned long long n_avail) {
    if (g + 16 <= n_avail) return *reinterpret_cast<const uint4 *>(in + g);
    unsigned v[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; i++)
        if (g + (unsigned)i < n_avail) v[i >> 2] |= (unsigned)in[g + (unsigned)i] << (8 * (i & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// the 16 positions from g on that lie in [entry, n_owned), as a mask
__device__ __forceinline__ unsigned tk_domain16(unsigned long long g, unsigned long long entry, unsigned long long n_owned) {
    const unsigned lo = entry > g ? (entry - g < 16 ? (unsigned)(entry - g) : 16u) : 0u;
    const unsigned hi = n_owned > g ? (n_owned - g < 16 ? (unsigned)(n_owned - g) : 16u) : 0u;
    return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

__global__ void __launch_bounds__(TK_WAVES * WAVE)
pfac_tk_count_kernel(const unsigned char *in, unsigned long long n_avail, const pfac_record *sel, unsigned long long n,
                     unsigned long long entry, unsigned long long n_owned, unsigned long long n_tiles, const short *flen,
                     const int *tok, const int *btok, unsigned num_final, const unsigned long long *first,
                     unsigned long long *bm, unsigned short *wpre, unsigned *tpre, unsigned long long *gsum,
                     unsigned long long *res) {
    __shared__ int s_btok[256];
    __shared__ unsigned long long s_cov[TK_WAVES][TK_WORDS], s_start[TK_WAVES][TK_WORDS], s_emit[TK_WAVES][TK_WORDS];
    __shared__ unsigned s_cnt[TK_GROUP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    s_btok[threadIdx.x] = btok[threadIdx.x];
    __syncthreads();
    bool bad = false;
    for (int i = 0; i < TK_GROUP / TK_WAVES; i++) {
        const unsigned lt = (unsigned)i * TK_WAVES + (unsigned)w;
        const unsigned long long t = (unsigned long long)blockIdx.x * TK_GROUP + lt;
        if (t >= n_tiles) {                                         // (wave-uniform)
            if (lane == 0) s_cnt[lt] = 0u;
            continue;
        }
        const unsigned long long tile_lo = t * WTILE, tile_hi = tile_lo + WTILE;
        const unsigned long long own_hi = tile_hi < n_owned ? tile_hi : n_owned;
        s_cov[w][lane] = 0ull;
        s_start[w][lane] = 0ull;
        wave_lds_sync();
        const unsigned long long f0 = first[t], f1 = first[t + 1];
        bad |= f0 > f1 || f1 > n;
        const unsigned long long k1 = f1 < n ? f1 : n;
        for (unsigned long long k = (f0 ? f0 - 1 : 0ull) + (unsigned)lane; k < k1; k += WAVE) {
            const pfac_record r = sel[k];
            const bool own = k >= f0;                               // else the pick in front of the tile's first
            const unsigned long long p = r.pos;
            int L = 0;
            bool drop = true;
            if (r.state < num_final) {
                L = flen[r.state];
                drop = tok[r.state] < 0;
            }
            if (own) {
                unsigned long long prev = entry;
                if (k > 0) {
                    const pfac_record q = sel[k - 1];
                    const int Lq = q.state < num_final ? (int)flen[q.state] : 0;
                    prev = (unsigned long long)q.pos + (unsigned long long)(Lq > 0 ? Lq : 0);
                }
                bad |= r.state >= num_final || L < 1 || p < tile_lo || p >= own_hi || p < prev;
                if (k + 1 == n) res[2] = p + (unsigned long long)(L > 0 ? L : 0);   // c_{n-1}
            }
            const unsigned long long a = p > tile_lo ? p : tile_lo;
            const unsigned long long e = p + (unsigned long long)(L > 0 ? L : 0);
            const unsigned long long b = e < tile_hi ? e : tile_hi;
            if (a < b) {                                            // at most 17 words: patterns are shorter than HALO_MAX
                const unsigned la = (unsigned)(a - tile_lo), lb = (unsigned)(b - tile_lo) - 1u;
                for (unsigned x = la >> 6; x <= lb >> 6; x++) {
                    unsigned long long m = ~0ull;
                    if (x == la >> 6) m &= ~tk_below(la & 63u);
                    if (x == lb >> 6 && (lb & 63u) != 63u) m &= tk_below((lb & 63u) + 1u);
                    atomicOr(&s_cov[w][x], m);
                }
                if (own && !drop && p >= tile_lo && p < tile_hi)
                    atomicOr(&s_start[w][(unsigned)(p - tile_lo) >> 6], 1ull << ((unsigned)(p - tile_lo) & 63u));
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < SUBS; j++) {
            const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
            const unsigned long long g = tile_lo + lp;
            const unsigned dom = tk_domain16(g, entry, n_owned);
            const unsigned cov = (unsigned)(s_cov[w][lp >> 6] >> sh) & 0xffffu;
            const unsigned st = (unsigned)(s_start[w][lp >> 6] >> sh) & 0xffffu;
            unsigned byte_bits = 0u;
            if (dom & ~cov) {
                const uint4 v = tk_load16(in, g, n_avail);
                const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int c = 0; c < 16; c++) byte_bits |= (unsigned)(s_btok[(q[c >> 2] >> (8 * (c & 3))) & 255u] >= 0) << c;
            }
            unsigned long long e = (unsigned long long)(((byte_bits & ~cov) | st) & dom) << sh;
            e |= __shfl_xor(e, 1, WAVE);
            e |= __shfl_xor(e, 2, WAVE);
            if ((lane & 3) == 0) s_emit[w][lp >> 6] = e;
        }
        wave_lds_sync();
        const unsigned long long word = s_emit[w][lane];
        const unsigned c = (unsigned)__popcll(word), incl = wave_incl_scan(c);
        bm[t * TK_WORDS + (unsigned)lane] = word;
        wpre[t * TK_WORDS + (unsigned)lane] = (unsigned short)(incl - c);
        if (lane == WAVE - 1) s_cnt[lt] = incl;
    }
    if (__ballot(bad) && lane == 0) atomicOr(&res[1], 1ull);
    __syncthreads();
    if (w == 0) {
        const unsigned long long t = (unsigned long long)blockIdx.x * TK_GROUP + (unsigned)lane;
        const unsigned c = s_cnt[lane], incl = wave_incl_scan(c);
        if (t < n_tiles) tpre[t] = incl - c;
        if (lane == WAVE - 1) gsum[blockIdx.x] = incl;
    }
}

template <bool POS>
__global__ void __launch_bounds__(WAVE)
pfac_tk_write_kernel(const unsigned char *in, unsigned long long n_avail, const pfac_record *sel, unsigned num_final,
                     const int *tok, const int *btok, const unsigned long long *first, const unsigned long long *bm,
                     const unsigned short *wpre, const unsigned *tpre, const unsigned long long *gpre, int *ids,
                     unsigned *pos) {
    __shared__ int s_btok[256];
    __shared__ unsigned long long s_bm[TK_WORDS];
    __shared__ unsigned short s_pre[TK_WORDS];
    __shared__ __attribute__((aligned(16))) int s_ids[TK_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned s_pos[POS ? TK_STAGE : 4];
    const int lane = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned long long word = bm[t * TK_WORDS + (unsigned)lane];
    const unsigned wp = wpre[t * TK_WORDS + (unsigned)lane];
    const unsigned cnt = bcast_last(wp + (unsigned)__popcll(word));
    if (cnt == 0) return;                                           // (wave-uniform)
    const unsigned long long base = gpre[t / TK_GROUP] + tpre[t];
    const unsigned a = (unsigned)(base & 3ull);
    const unsigned long long tile_lo = t * WTILE;
    s_bm[lane] = word;
    s_pre[lane] = (unsigned short)wp;
#pragma unroll
    for (int i = 0; i < 4; i++) s_btok[i * WAVE + lane] = btok[i * WAVE + lane];
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < SUBS; j++) {                                // the byte tokens, in rank order
        const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
        const unsigned long long wv = s_bm[lp >> 6];
        unsigned e = (unsigned)(wv >> sh) & 0xffffu;
        if (!e) continue;
        unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(sh));
        const uint4 v = tk_load16(in, tile_lo + lp, n_avail);
        const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (e >> c & 1u) {
                s_ids[rank] = s_btok[(q[c >> 2] >> (8 * (c & 3))) & 255u];
                if constexpr (POS) s_pos[rank] = (unsigned)(tile_lo + lp + (unsigned)c);
                rank++;
            }
        }
    }
    wave_lds_sync();
    const unsigned long long f1 = first[t + 1];
    for (unsigned long long k = first[t] + (unsigned)lane; k < f1; k += WAVE) {     // the kept picks, over their bytes
        const pfac_record r = sel[k];
        const unsigned lp = (r.pos - (unsigned)tile_lo) & (WTILE - 1u);
        const unsigned long long wv = s_bm[lp >> 6];
        const int v = r.state < num_final ? tok[r.state] : -1;
        if (v >= 0 && (wv >> (lp & 63u) & 1ull)) {
            const unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(lp & 63u));
            s_ids[rank] = v;
            if constexpr (POS) s_pos[rank] = (unsigned)tile_lo + lp;
        }
    }
    wave_lds_sync();
    const unsigned long long g0 = base - a;                         // a multiple of 4: ids + g0 is 16-B aligned
    for (unsigned c = (unsigned)lane; c * 4u < a + cnt; c += WAVE) {
        const unsigned s0 = c * 4u;
        if (s0 >= a && s0 + 4u <= a + cnt) {
            *reinterpret_cast<uint4 *>(ids + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_ids[s0]);
            if constexpr (POS) *reinterpret_cast<uint4 *>(pos + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_pos[s0]);
        } else {
            for (unsigned x = s0; x < s0 + 4u; x++) {
                if (x >= a && x < a + cnt) {
                    ids[g0 + x] = s_ids[x];
                    if constexpr (POS) pos[g0 + x] = s_pos[x];
                }
            }
        }
    }
}

__global__ void pfac_tk_doc_kernel(const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                                   unsigned long long n_tiles, unsigned n_groups, const unsigned long long *bm,
                                   const unsigned short *wpre, const unsigned *tpre, const unsigned long long *gpre,
                                   unsigned long long *tok_off) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
        const unsigned long long o = off[d], t = o >> 12;
        unsigned long long v = gpre[n_groups];                      // the total: off[d] == n_owned (or no tile at all)
        if (o < n_owned && t < n_tiles) {
            const unsigned x = (unsigned)(o & (WTILE - 1u)) >> 6;
            v = gpre[t / TK_GROUP] + tpre[t] + wpre[t * TK_WORDS + x] +
                (unsigned long long)__popcll(bm[t * TK_WORDS + x] & tk_below((unsigned)o & 63u));
        }
        tok_off[d] = v;
    }
}

// ---------------------------------------------------------------------------
// WordPiece (pfac_table_set_wordpiece, pfac_records_filter_roles, pfac_wordpiece_leftmost_longest / _documents).  One
// automaton over the stripped strings; every final state has a pair of ids, .x for a piece at a word's start (FIRST),
// .y for one inside a word (CONT).  role(p) depends on the input alone: CONT iff p > 0 and in[p - 1] is a word byte.
//
// Role filter (pfac_filter_roles_kernel): the walk of pfac_filter_words_kernel -- a wave per tile at a time, 64 tiles
// per wave, chunks of 64 records, a ballot, the kept words stored at or below their own slots (in place is safe for the
// reason given there).  Per record two byte gathers (p - 1, p) and one 8-byte gather of the id pair; kept iff in[p] is a
// word byte and the id of role(p) is not DROP.
template <int BYTES>
__global__ void pfac_filter_roles_kernel(void *rec, unsigned long long *tix, unsigned long long n_tiles, unsigned long long cap,
                                         const unsigned char *in, unsigned long long n_avail, const int2 *ids,
                                         unsigned num_final, WordSet ws, unsigned long long *total) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    if (g >= n_groups) return;
    const unsigned long long t = (unsigned long long)g * XGROUP + lane;
    const unsigned long long e = t < n_tiles ? tix[t] : 0ull;
    const unsigned c = (unsigned)(e >> TIX_CNT_SHIFT);
    const unsigned long long lo = e & TIX_BASE_MASK;
    unsigned mine = c;                                          // records tile t keeps
    for (int j = 0; j < XGROUP; j++) {
        const unsigned tc = __shfl(c, j, WAVE);
        if (tc == 0) continue;
        const unsigned long long tlo = __shfl(lo, j, WAVE);
        unsigned kept = 0;
        for (unsigned c0 = 0; c0 < tc; c0 += WAVE) {
            const unsigned i = c0 + (unsigned)lane;
            const bool have = i < tc && tlo + i < cap;
            unsigned pos = 0, st = 0;
            if (have) heap_record<BYTES>(rec, tlo + i, (unsigned long long)g * XGROUP + j, pos, st);
            bool keep = false;
            if (have && st < num_final && pos < n_avail && word_byte(ws, (int)in[pos])) {
                const bool cont = pos > 0 && word_byte(ws, (int)in[pos - 1]);
                const int2 pr = ids[st];
                keep = (cont ? pr.y : pr.x) >= 0;
            }
            const unsigned long long b = __ballot(keep);
            const unsigned to = kept + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
            if (keep && to != i) heap_put<BYTES>(rec, tlo + to, pos, st);
            kept += (unsigned)__popcll(b);
        }
        if (lane == j) mine = kept;
    }
    if (t < n_tiles && mine != c) tix[t] = lo | (unsigned long long)mine << TIX_CNT_SHIFT;
    const unsigned long long sum = wave_sum64(mine);
    if (lane == 0 && sum) atomicAdd(total, sum);
}

// Token pass.  A word is a maximal run of word bytes inside [0, n_owned); it is good iff it is at most max_word bytes
// long and every byte of it is covered by a pick.  Positions emit: the first byte of a bad word unk_id; a pick start
// inside a good word the id of its role (unless DROP); a non-word byte outside every pick btok[byte] (unless DROP).
//   pfac_tk_first_kernel     the tokenizer's, unchanged
//   pfac_wp_edge_kernel      one wave per tile.  Four bitmaps of the tile's 4096 positions, KEPT for the count pass
//                            (2 KiB per tile; it neither loads the input nor walks the picks again): W word bytes
//                            below n_owned, U = W & ~covered, ST the own pick starts on a word byte whose role id is
//                            kept, E0 the non-word bytes outside every pick whose btok is kept.  And the tile's edge
//                            summary, four 16-bit fields: the length of the leading run of W and bit 15 = it holds a
//                            bit of U; the same for the trailing run.  The d_sel checks of pfac_tk_count_kernel ride
//                            along (each pick by the tile that owns its start).
//   pfac_wp_count_kernel     a workgroup per 64 tiles, a wave per tile at a time, a lane per bitmap word; no LDS but the
//                            tile counts.  max_word <= 4095, so a word touches at most two tiles unless it fills one
//                            (then it is bad by itself): the verdict of a run on a tile edge needs the NEIGHBOUR's
//                            summary only -- no scan over tiles.  Seeds of "bad": U; the edge bit of a run the
//                            neighbour's summary condemns (its part is uncovered, or the two parts are too long
//                            together); and every position that ends max_word + 1 word bits in a row -- found from the
//                            run length that reaches each word's bit 0 (a segmented scan over the 64 lanes: + 64 per
//                            full word) and, for max_word < 64, the AND of max_word + 1 shifted copies of the word by
//                            doubling.  The seeds flood along W upwards and downwards: a Kogge-Stone fill inside the
//                            64-bit word, the carries between the lanes by the same fill over the ballots of
//                            "reaches bit 63 / bit 0" and "all ones".  bad & word start = the [UNK] positions;
//                            emits = E0 | unk | ST & ~bad.  Kept: bm, wpre, tpre, gsum as the tokenizer keeps them (so
//                            pfac_scan_groups_kernel and pfac_tk_doc_kernel serve unchanged), and the unk bitmap.
//   pfac_wp_write_kernel     pfac_tk_write_kernel with two changes: the byte stage writes unk_id at the positions of
//                            the unk bitmap; the pick stage skips those and takes .x or .y by the W bit in front of
//                            the pick (one byte gather in front of the tile for its first position).
//   pfac_wp_docs_kernel      one thread per document offset: 0, n_owned, or a non-word byte on one side of it.
// No loop's trip count is the length of a word, a gap or a run of documents.
constexpr int WP_MAPS = 4;                          // W, U, ST, E0
constexpr unsigned WP_LEN = 0x7fffu, WP_BAD = 0x8000u;          // a summary field: run length (0..4096) | uncovered

// the bits of word x (tile positions 64 x ..) that lie in [lo, hi)
__device__ __forceinline__ unsigned long long wp_range(unsigned x, unsigned lo, unsigned hi) {
    const unsigned b = x * 64u;
    const unsigned a = lo > b ? lo - b : 0u, e = hi > b ? hi - b : 0u;
    const unsigned long long ma = a >= 64u ? ~0ull : tk_below(a), me = e >= 64u ? ~0ull : tk_below(e);
    return me & ~ma;
}
__device__ __forceinline__ unsigned long long wp_fill_up(unsigned long long g, unsigned long long p) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        g |= p & (g << sh);
        p &= p << sh;
    }
    return g;
}
__device__ __forceinline__ unsigned long long wp_fill_down(unsigned long long g, unsigned long long p) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        g |= p & (g >> sh);
        p &= p >> sh;
    }
    return g;
}

__global__ void __launch_bounds__(WAVE)
pfac_wp_edge_kernel(const unsigned char *in, unsigned long long n_avail, const pfac_record *sel, unsigned long long n,
                    unsigned long long n_owned, const short *flen, const int2 *ids, const int *btok, unsigned num_final,
                    const unsigned long long *first, WordSet ws, unsigned long long *maps, unsigned long long *sum,
                    unsigned long long *res) {
    __shared__ unsigned long long s_w[TK_WORDS], s_e0[TK_WORDS], s_cov[TK_WORDS], s_start[TK_WORDS];
    const int lane = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned long long tile_lo = t * WTILE, tile_hi = tile_lo + WTILE;
    const unsigned long long own_hi = tile_hi < n_owned ? tile_hi : n_owned;
    WordSet bv;                                                     // the non-word bytes whose btok is kept
#pragma unroll
    for (int k = 0; k < 4; k++) bv.w[k] = __ballot(btok[k * WAVE + lane] >= 0) & ~ws.w[k];
    s_cov[lane] = 0ull;
    s_start[lane] = 0ull;
#pragma unroll
    for (int j = 0; j < SUBS; j++) {
        const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
        const unsigned long long g = tile_lo + lp;
        const unsigned dom = tk_domain16(g, 0ull, n_owned);
        unsigned wb = 0u, nb = 0u;
        if (dom) {
            const uint4 v = tk_load16(in, g, n_avail);
            const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const int byte = (int)((q[c >> 2] >> (8 * (c & 3))) & 255u);
                wb |= (unsigned)word_byte(ws, byte) << c;
                nb |= (unsigned)word_byte(bv, byte) << c;
            }
        }
        unsigned long long a = (unsigned long long)(wb & dom) << sh, b = (unsigned long long)(nb & dom) << sh;
        a |= __shfl_xor(a, 1, WAVE);
        a |= __shfl_xor(a, 2, WAVE);
        b |= __shfl_xor(b, 1, WAVE);
        b |= __shfl_xor(b, 2, WAVE);
        if ((lane & 3) == 0) {
            s_w[lp >> 6] = a;
            s_e0[lp >> 6] = b;
        }
    }
    wave_lds_sync();
    const bool cont0 = t > 0 && word_byte(ws, (int)in[tile_lo - 1]);       // (tile_lo < n_owned <= n_avail)
    bool bad = false;
    const unsigned long long f0 = first[t], f1 = first[t + 1];
    bad |= f0 > f1 || f1 > n;
    const unsigned long long k1 = f1 < n ? f1 : n;
    for (unsigned long long k = (f0 ? f0 - 1 : 0ull) + (unsigned)lane; k < k1; k += WAVE) {
        const pfac_record r = sel[k];
        const bool own = k >= f0;                                   // else the pick in front of the tile's first
        const unsigned long long p = r.pos;
        const int L = r.state < num_final ? (int)flen[r.state] : 0;
        if (own) {
            unsigned long long prev = 0ull;
            if (k > 0) {
                const pfac_record q = sel[k - 1];
                const int Lq = q.state < num_final ? (int)flen[q.state] : 0;
                prev = (unsigned long long)q.pos + (unsigned long long)(Lq > 0 ? Lq : 0);
            }
            bad |= r.state >= num_final || L < 1 || p < tile_lo || p >= own_hi || p < prev;
            if (k + 1 == n) res[2] = p + (unsigned long long)(L > 0 ? L : 0);       // c_{n-1}
        }
        const unsigned long long a = p > tile_lo ? p : tile_lo;
        const unsigned long long e = p + (unsigned long long)(L > 0 ? L : 0);
        const unsigned long long b = e < tile_hi ? e : tile_hi;
        if (a < b) {                                                // at most 17 words: patterns are shorter than HALO_MAX
            const unsigned la = (unsigned)(a - tile_lo), lb = (unsigned)(b - tile_lo) - 1u;
            for (unsigned x = la >> 6; x <= lb >> 6; x++) {
                unsigned long long m = ~0ull;
                if (x == la >> 6) m &= ~tk_below(la & 63u);
                if (x == lb >> 6 && (lb & 63u) != 63u) m &= tk_below((lb & 63u) + 1u);
                atomicOr(&s_cov[x], m);
            }
            if (own && r.state < num_final && p >= tile_lo && p < own_hi) {
                const unsigned lp = (unsigned)(p - tile_lo);
                const bool cont = lp ? (s_w[(lp - 1u) >> 6] >> ((lp - 1u) & 63u) & 1ull) != 0ull : cont0;
                const int2 pr = ids[r.state];
                if ((cont ? pr.y : pr.x) >= 0) atomicOr(&s_start[lp >> 6], 1ull << (lp & 63u));
            }
        }
    }
    if (__ballot(bad) && lane == 0) atomicOr(&res[1], 1ull);
    wave_lds_sync();
    const unsigned long long W = s_w[lane], cov = s_cov[lane], U = W & ~cov;
    unsigned long long *m = maps + t * (WP_MAPS * TK_WORDS);
    m[lane] = W;
    m[TK_WORDS + lane] = U;
    m[2 * TK_WORDS + lane] = s_start[lane] & W;
    m[3 * TK_WORDS + lane] = s_e0[lane] & ~cov;
    const unsigned long long open = __ballot(W != ~0ull);          // the words that end a run
    unsigned lead = WTILE, trail = WTILE;
    if (open) {
        const int x0 = __builtin_ctzll(open), x1 = 63 - __builtin_clzll(open);
        const unsigned long long w0 = __shfl(W, x0, WAVE), w1 = __shfl(W, x1, WAVE);
        lead = (unsigned)x0 * 64u + (unsigned)__builtin_ctzll(~w0);
        trail = (unsigned)(63 - x1) * 64u + (unsigned)__builtin_clzll(~w1);
    }
    const bool lbad = __ballot((U & wp_range((unsigned)lane, 0u, lead)) != 0ull) != 0ull;
    const bool tbad = __ballot((U & wp_range((unsigned)lane, WTILE - trail, WTILE)) != 0ull) != 0ull;
    if (lane == 0)
        sum[t] = (unsigned long long)(lead | (lbad ? WP_BAD : 0u)) | (unsigned long long)(trail | (tbad ? WP_BAD : 0u)) << 16;
}

__global__ void __launch_bounds__(TK_WAVES * WAVE)
pfac_wp_count_kernel(const unsigned long long *maps, const unsigned long long *sum, unsigned long long n_tiles, unsigned max_word,
                     unsigned long long *bm, unsigned long long *unk, unsigned short *wpre, unsigned *tpre,
                     unsigned long long *gsum) {
    __shared__ unsigned s_cnt[TK_GROUP];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const unsigned K = max_word + 1u;                               // so many word bits in a row make a word too long
    for (int i = 0; i < TK_GROUP / TK_WAVES; i++) {
        const unsigned lt = (unsigned)i * TK_WAVES + (unsigned)w;
        const unsigned long long t = (unsigned long long)blockIdx.x * TK_GROUP + lt;
        if (t >= n_tiles) {                                         // (wave-uniform)
            if (lane == 0) s_cnt[lt] = 0u;
            continue;
        }
        const unsigned long long *m = maps + t * (WP_MAPS * TK_WORDS);
        const unsigned long long W = m[lane], U = m[TK_WORDS + lane], ST = m[2 * TK_WORDS + lane], E0 = m[3 * TK_WORDS + lane];
        const unsigned sm = (unsigned)sum[t], prev = t ? (unsigned)sum[t - 1] : 0u, next = t + 1 < n_tiles ? (unsigned)sum[t + 1] : 0u;
        const unsigned lead = sm & WP_LEN, trail = sm >> 16 & WP_LEN;
        const unsigned ptrail = prev >> 16 & WP_LEN, nlead = next & WP_LEN;
        // a run on a tile edge that goes on in the neighbour: what the neighbour's part adds to the verdict
        const bool seed_lo = lead && ptrail && (lead == WTILE || ptrail == WTILE || lead + ptrail > max_word || (prev >> 16 & WP_BAD));
        const bool seed_hi = trail && nlead && (trail == WTILE || nlead == WTILE || trail + nlead > max_word || (next & WP_BAD));
        // word bits in a row up to and including bit 63 of every word; cin = those that reach this word's bit 0
        const bool full = W == ~0ull;
        const unsigned lowrun = full ? 64u : (unsigned)__builtin_ctzll(~W);
        unsigned v = full ? 64u : (unsigned)__builtin_clzll(~W);
        unsigned f = full ? 0u : 1u;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned pv = __shfl_up(v, d, WAVE), pf = __shfl_up(f, d, WAVE);
            if (lane >= d && !f) {
                v += pv;
                f = pf;
            }
        }
        unsigned cin = __shfl_up(v, 1, WAVE);
        if (lane == 0) cin = 0u;
        unsigned long long S = U;
        if (cin + lowrun > max_word) S |= wp_range(0u, max_word > cin ? max_word - cin : 0u, lowrun);
        if (K <= 64u) {                                             // (uniform) runs of K inside the word
            unsigned long long acc = ~0ull, pw = W;
            unsigned am = 0u;
            for (unsigned bit = 0; bit < 7u; bit++) {
                if (K >> bit & 1u) {
                    acc &= pw << am;
                    am += 1u << bit;
                }
                if (bit < 6u) pw &= pw << (1u << bit);
            }
            S |= acc;
        }
        if (seed_lo && lane == 0) S |= 1ull;
        if (seed_hi && lane == WAVE - 1) S |= 1ull << 63;
        S &= W;
        unsigned long long up = wp_fill_up(S, W), dn = wp_fill_down(S, W);
        const unsigned long long P = __ballot(full);
        const unsigned long long cu = wp_fill_up(__ballot(up >> 63 != 0ull) << 1, P << 1);
        const unsigned long long cd = wp_fill_down(__ballot((dn & 1ull) != 0ull) >> 1, P >> 1);
        if (cu >> lane & 1ull) up |= W & ~(W + 1ull);               // the carry from below floods the run at bit 0
        if (cd >> lane & 1ull) dn |= full ? ~0ull : ~(~0ull >> __builtin_clzll(~W));   // ... from above, the run at bit 63
        const unsigned long long bad = up | dn;
        unsigned top = (unsigned)(W >> 63);
        top = __shfl_up(top, 1, WAVE);
        if (lane == 0) top = ptrail ? 1u : 0u;
        const unsigned long long ws_ = W & ~(W << 1 | (unsigned long long)top);
        const unsigned long long uk = ws_ & bad;
        const unsigned long long word = E0 | uk | (ST & ~bad);
        const unsigned c = (unsigned)__popcll(word), incl = wave_incl_scan(c);
        bm[t * TK_WORDS + (unsigned)lane] = word;
        unk[t * TK_WORDS + (unsigned)lane] = uk;
        wpre[t * TK_WORDS + (unsigned)lane] = (unsigned short)(incl - c);
        if (lane == WAVE - 1) s_cnt[lt] = incl;
    }
    __syncthreads();
    if (w == 0) {
        const unsigned long long t = (unsigned long long)blockIdx.x * TK_GROUP + (unsigned)lane;
        const unsigned c = s_cnt[lane], incl = wave_incl_scan(c);
        if (t < n_tiles) tpre[t] = incl - c;
        if (lane == WAVE - 1) gsum[blockIdx.x] = incl;
    }
}

template <bool POS>
__global__ void __launch_bounds__(WAVE)
pfac_wp_write_kernel(const unsigned char *in, unsigned long long n_avail, const pfac_record *sel, unsigned num_final,
                     const int2 *pids, const int *btok, int unk_id, WordSet ws, const unsigned long long *first,
                     const unsigned long long *maps, const unsigned long long *bm, const unsigned long long *unk,
                     const unsigned short *wpre, const unsigned *tpre, const unsigned long long *gpre, int *ids, unsigned *pos) {
    __shared__ int s_btok[256];
    __shared__ unsigned long long s_bm[TK_WORDS], s_unk[TK_WORDS], s_w[TK_WORDS];
    __shared__ unsigned short s_pre[TK_WORDS];
    __shared__ __attribute__((aligned(16))) int s_ids[TK_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned s_pos[POS ? TK_STAGE : 4];
    const int lane = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned long long word = bm[t * TK_WORDS + (unsigned)lane];
    const unsigned wp = wpre[t * TK_WORDS + (unsigned)lane];
    const unsigned cnt = bcast_last(wp + (unsigned)__popcll(word));
    if (cnt == 0) return;                                           // (wave-uniform)
    const unsigned long long base = gpre[t / TK_GROUP] + tpre[t];
    const unsigned a = (unsigned)(base & 3ull);
    const unsigned long long tile_lo = t * WTILE;
    s_bm[lane] = word;
    s_unk[lane] = unk[t * TK_WORDS + (unsigned)lane];
    s_w[lane] = maps[t * (WP_MAPS * TK_WORDS) + (unsigned)lane];
    s_pre[lane] = (unsigned short)wp;
#pragma unroll
    for (int i = 0; i < 4; i++) s_btok[i * WAVE + lane] = btok[i * WAVE + lane];
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < SUBS; j++) {                                // the byte and [UNK] tokens, in rank order
        const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
        const unsigned long long wv = s_bm[lp >> 6];
        unsigned e = (unsigned)(wv >> sh) & 0xffffu;
        if (!e) continue;
        const unsigned u = (unsigned)(s_unk[lp >> 6] >> sh) & 0xffffu;
        unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(sh));
        const uint4 v = tk_load16(in, tile_lo + lp, n_avail);
        const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (e >> c & 1u) {
                s_ids[rank] = (u >> c & 1u) ? unk_id : s_btok[(q[c >> 2] >> (8 * (c & 3))) & 255u];
                if constexpr (POS) s_pos[rank] = (unsigned)(tile_lo + lp + (unsigned)c);
                rank++;
            }
        }
    }
    wave_lds_sync();
    const bool cont0 = t > 0 && word_byte(ws, (int)in[tile_lo - 1]);
    const unsigned long long f1 = first[t + 1];
    for (unsigned long long k = first[t] + (unsigned)lane; k < f1; k += WAVE) {     // the kept picks of good words
        const pfac_record r = sel[k];
        const unsigned lp = (r.pos - (unsigned)tile_lo) & (WTILE - 1u);
        const unsigned long long wv = s_bm[lp >> 6];
        if (r.state < num_final && (wv >> (lp & 63u) & 1ull) && !(s_unk[lp >> 6] >> (lp & 63u) & 1ull)) {
            const bool cont = lp ? (s_w[(lp - 1u) >> 6] >> ((lp - 1u) & 63u) & 1ull) != 0ull : cont0;
            const int2 pr = pids[r.state];
            const int v = cont ? pr.y : pr.x;
            if (v >= 0) {
                const unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(lp & 63u));
                s_ids[rank] = v;
                if constexpr (POS) s_pos[rank] = (unsigned)tile_lo + lp;
            }
        }
    }
    wave_lds_sync();
    const unsigned long long g0 = base - a;                         // a multiple of 4: ids + g0 is 16-B aligned
    for (unsigned c = (unsigned)lane; c * 4u < a + cnt; c += WAVE) {
        const unsigned s0 = c * 4u;
        if (s0 >= a && s0 + 4u <= a + cnt) {
            *reinterpret_cast<uint4 *>(ids + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_ids[s0]);
            if constexpr (POS) *reinterpret_cast<uint4 *>(pos + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_pos[s0]);
        } else {
            for (unsigned x = s0; x < s0 + 4u; x++) {
                if (x >= a && x < a + cnt) {
                    ids[g0 + x] = s_ids[x];
                    if constexpr (POS) pos[g0 + x] = s_pos[x];
                }
            }
        }
    }
}

// every document offset on a word boundary (two byte loads per offset, both below n_owned); else bit 1 of *err
__global__ void pfac_wp_docs_kernel(const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                                    const unsigned char *in, WordSet ws, unsigned long long *err) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    bool bad = false;
    for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
        const unsigned long long o = off[d];
        if (o > 0 && o < n_owned) bad |= word_byte(ws, (int)in[o - 1]) && word_byte(ws, (int)in[o]);
    }
    if (bad) atomicOr(err, 2ull);
}

// ---------------------------------------------------------------------------
// Unigram (pfac_table_set_unigram, pfac_unigram_records / _documents): the best-scoring cut of every word, by Viterbi
// over the lattice of ALL records inside the word (THE RULE is in pfac.h).  The first token pass that reads the record
// heap, not a selection.  Position-driven over the scan's 4 KiB tiles; no dependency between tiles.
//   pfac_ug_solve_kernel     a workgroup of four waves per tile.  Its region is the tile and EXT bytes on either side
//                            (EXT = 256 for max_word <= 255, else 4096; EXT > max_word, so the region holds every word
//                            of at most max_word bytes that touches the tile, whole).  In LDS, by region position: the
//                            bitmaps W (word bytes below n_owned) and K (bytes whose byte id is kept), 16 bytes per lane
//                            per load; S (edge starts of the chosen paths) and B (byte edges), which start as W -- a
//                            word nobody solves (over the cap, or with its start further back than EXT, which is over
//                            the cap too) is all byte edges.  The word starts of the region that lie in front of the
//                            tile's end are listed in LDS and dealt to the lanes, one word per lane at a time: the
//                            word's end from W, then a forward DP over best[] (int32) and the chosen edge (uint16:
//                            length | UG_BYTE) -- the records of position i pushed in heap order, which is ascending
//                            length, then the byte edge, each with a strict >, which IS the tie rule -- then the
//                            backtrack, which clears S inside and B over every piece edge.  The lane finds the first
//                            record of its word by one binary search in the tile's run and then walks the run (and the
//                            next tile's) in step with the positions: trip count = the word's bytes + its records.  A
//                            word that straddles a tile edge is solved by both tiles, from the same bytes and records:
//                            they agree.  Then one wave derives the tile's emitting positions from the four bitmaps
//                            (unk fusing needs B of the position in front: the region has it) and keeps W, S, B, the
//                            emit bitmap, the 16-bit prefix per word and the tile's count.
//   pfac_ug_group_kernel     one wave per 64 tiles: the counts become the prefixes inside the group, and its sum
//   pfac_scan_groups_kernel, pfac_wp_docs_kernel, pfac_tk_doc_kernel: unchanged
//   pfac_ug_write_kernel     one wave per tile, pfac_tk_write_kernel's staging and stores.  Byte and unk tokens first;
//                            then "first record of position p" (LDS, one lane per record) and a lane per bitmap word
//                            over its piece starts: a piece runs to the next edge start or the word's end (the next bit
//                            of S | ~W, in the next tile's maps where it straddles), its state is the record (p, L).
constexpr int UG_THREADS = 4 * WAVE;
constexpr int UG_MAPS = 3;                          // W, S, B
constexpr unsigned UG_BYTE = 0x8000u;               // chosen edge: the byte edge (else a piece of that length)
constexpr int UG_NEG = -2147483647 - 1;             // best[] of a node nothing has reached yet

// bits [lo, hi) of the 64-bit words of an LDS bitmap cleared (lo < hi)
__device__ __forceinline__ void ug_clear(unsigned long long *m, unsigned lo, unsigned hi) {
    for (unsigned x = lo >> 6; x <= (hi - 1u) >> 6; x++) atomicAnd(&m[x], ~wp_range(x, lo, hi));
}

struct UgRun {                                      // a tile's run of the heap
    unsigned long long base;
    unsigned cnt;
};
__device__ __forceinline__ UgRun ug_run_of(const unsigned long long *tix, unsigned long long n_tix, unsigned long long cap,
                                           unsigned long long t) {
    UgRun r{0ull, 0u};
    if (t < n_tix) {
        const unsigned long long e = tix[t];
        r.base = e & TIX_BASE_MASK;
        r.cnt = (unsigned)(e >> TIX_CNT_SHIFT);
        if (r.base >= cap) r.cnt = 0u;                              // (records past the capacity were never written)
        else if (r.base + r.cnt > cap) r.cnt = (unsigned)(cap - r.base);
    }
    return r;
}

template <int BYTES, int EXT>
__global__ void __launch_bounds__(UG_THREADS)
pfac_ug_solve_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tix, unsigned long long cap,
                     const unsigned char *in, unsigned long long n_avail, unsigned long long n_owned, const short *flen,
                     const int4 *pieces, const int *btok, unsigned num_final, int byte_score, int unk_id, unsigned max_word,
                     WordSet ws, unsigned long long *maps, unsigned long long *bm, unsigned short *wpre, unsigned *tcnt) {
    constexpr unsigned R = WTILE + 2 * EXT, RW = R / 64;
    __shared__ int s_best[R];
    __shared__ unsigned short s_ch[R];
    __shared__ unsigned short s_list[R / 2 + 64];
    __shared__ unsigned long long s_W[RW], s_K[RW], s_S[RW], s_B[RW];
    __shared__ unsigned s_n;
    const unsigned tid = threadIdx.x;
    const int lane = (int)(tid & (WAVE - 1));
    const unsigned long long t = blockIdx.x;
    const unsigned long long tile_lo = t * WTILE;
    const unsigned off0 = t ? (unsigned)EXT : 0u;                   // the tile's first position in the region
    const unsigned long long reg_lo = tile_lo - off0;
    WordSet kv;                                                     // the bytes whose byte id is kept
#pragma unroll
    for (int k = 0; k < 4; k++) kv.w[k] = __ballot(btok[k * WAVE + lane] >= 0);
    if (tid == 0) s_n = 0u;
    for (unsigned c = tid; c < R / 16; c += UG_THREADS) {
        const unsigned long long g = reg_lo + c * 16ull;
        const unsigned dom = tk_domain16(g, 0ull, n_owned);
        unsigned wb = 0u, kb = 0u;
        if (dom) {
            const uint4 v = tk_load16(in, g, n_avail);
            const auto four = [&](unsigned q, int at) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int byte = (int)((q >> (8 * i)) & 255u);
                    wb |= (unsigned)word_byte(ws, byte) << (at + i);
                    kb |= (unsigned)word_byte(kv, byte) << (at + i);
                }
            };
            four(v.x, 0);
            four(v.y, 4);
            four(v.z, 8);
            four(v.w, 12);
        }
        reinterpret_cast<unsigned short *>(s_W)[c] = (unsigned short)(wb & dom);
        reinterpret_cast<unsigned short *>(s_K)[c] = (unsigned short)(kb & dom);
    }
    for (unsigned r = tid; r < R; r += UG_THREADS) s_best[r] = UG_NEG;
    __syncthreads();
    for (unsigned x = tid; x < RW; x += UG_THREADS) {
        const unsigned long long W = s_W[x];
        s_S[x] = W;
        s_B[x] = W;
        // a start: a word byte with none in front of it; what lies in front of the region is not known (taken as one)
        const unsigned long long top = x ? s_W[x - 1] >> 63 : (reg_lo ? 1ull : 0ull);
        unsigned long long st = W & ~(W << 1 | top);
        if (x * 64u >= off0 + WTILE) st = 0ull;                     // the words that start behind the tile are not its own
        while (st) {
            const unsigned b = (unsigned)__builtin_ctzll(st);
            st &= st - 1ull;
            s_list[atomicAdd(&s_n, 1u)] = (unsigned short)(x * 64u + b);
        }
    }
    __syncthreads();
    const unsigned n_words = s_n;
    for (unsigned k = tid; k < n_words; k += UG_THREADS) {
        const unsigned a = s_list[k];
        unsigned b = R;                                             // the word's end: the first 0 of W behind a
        {
            unsigned x = a >> 6;
            unsigned long long inv = ~s_W[x] & ~tk_below(a & 63u);
            while (!inv && x + 1u < RW && (x + 1u) * 64u <= a + max_word) inv = ~s_W[++x];
            if (inv) b = x * 64u + (unsigned)__builtin_ctzll(inv);
        }
        if (b - a > max_word || b <= off0) continue;                // over the cap: all byte edges, as S and B stand
        const unsigned long long ga = reg_lo + a;
        unsigned long long ct = ga >> 12;
        UgRun run = ug_run_of(tix, n_tix, cap, ct);
        unsigned j = 0;
        {                                                           // the first record at or behind a
            unsigned hi = run.cnt;
            while (j < hi) {
                const unsigned m = j + (hi - j) / 2u;
                unsigned p, s;
                heap_record<BYTES>(rec, run.base + m, ct, p, s);
                if ((unsigned long long)p < ga) j = m + 1u;
                else hi = m;
            }
        }
        unsigned rp = 0u, rs = 0u;
        bool have = false;
        s_best[a] = 0;
        for (unsigned i = a; i < b; i++) {
            const unsigned long long gi = reg_lo + i;
            if (gi >> 12 != ct) {                                   // the word goes on in the next tile: its run
                ct = gi >> 12;
                run = ug_run_of(tix, n_tix, cap, ct);
                j = 0u;
                have = false;
            }
            const int bi = s_best[i];
            for (;;) {
                if (!have) {
                    if (j >= run.cnt) break;
                    heap_record<BYTES>(rec, run.base + j, ct, rp, rs);
                    have = true;
                }
                if ((unsigned long long)rp != gi) break;
                have = false;
                j++;
                if (rs >= num_final) continue;
                const int L = flen[rs];
                if (L < 1 || i + (unsigned)L > b) continue;
                const int4 pc = pieces[rs];
                const int id = i == a ? pc.x : pc.y, sc = i == a ? pc.z : pc.w;
                if (id < 0) continue;
                if (bi + sc > s_best[i + (unsigned)L]) {
                    s_best[i + (unsigned)L] = bi + sc;
                    s_ch[i + (unsigned)L] = (unsigned short)L;
                }
            }
            if (bi + byte_score > s_best[i + 1u]) {
                s_best[i + 1u] = bi + byte_score;
                s_ch[i + 1u] = (unsigned short)(1u | UG_BYTE);
            }
        }
        for (unsigned e = b; e > a;) {                              // the path, from its end
            const unsigned c = s_ch[e], L = c & 0x7fffu, p = e - L;
            if (!(c & UG_BYTE)) {
                ug_clear(s_B, p, e);
                if (L > 1u) ug_clear(s_S, p + 1u, e);
            }
            e = p;
        }
    }
    __syncthreads();
    if (tid < WAVE) {
        const unsigned x = off0 / 64u + (unsigned)lane;
        const unsigned long long W = s_W[x], K = s_K[x], S = s_S[x], B = s_B[x];
        const unsigned long long prevb = x ? s_B[x - 1] >> 63 : 0ull;
        const unsigned long long ub = unk_id >= 0 ? B & ~(B << 1 | prevb) : B & K;
        const unsigned long long word = (K & ~W) | (S & ~B) | ub;
        const unsigned c = (unsigned)__popcll(word), incl = wave_incl_scan(c);
        unsigned long long *m = maps + t * (UG_MAPS * TK_WORDS);
        m[lane] = W;
        m[TK_WORDS + lane] = S;
        m[2 * TK_WORDS + lane] = B;
        bm[t * TK_WORDS + (unsigned)lane] = word;
        wpre[t * TK_WORDS + (unsigned)lane] = (unsigned short)(incl - c);
        if (lane == WAVE - 1) tcnt[t] = incl;
    }
}

// the tiles' counts -> the tokens in front of each tile in its group of 64, and the group's sum
__global__ void __launch_bounds__(WAVE)
pfac_ug_group_kernel(unsigned *tpre, unsigned long long n_tiles, unsigned long long *gsum) {
    const unsigned long long t = (unsigned long long)blockIdx.x * TK_GROUP + threadIdx.x;
    const unsigned c = t < n_tiles ? tpre[t] : 0u, incl = wave_incl_scan(c);
    if (t < n_tiles) tpre[t] = incl - c;
    if (threadIdx.x == WAVE - 1) gsum[blockIdx.x] = incl;
}

template <int BYTES, bool POS>
__global__ void __launch_bounds__(WAVE)
pfac_ug_write_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tix, unsigned long long cap,
                     const unsigned char *in, unsigned long long n_avail, const short *flen, const int4 *pieces,
                     const int *btok, unsigned num_final, int unk_id, WordSet ws, const unsigned long long *maps,
                     unsigned long long n_tiles, const unsigned long long *bm, const unsigned short *wpre,
                     const unsigned *tpre, const unsigned long long *gpre, int *ids, unsigned *pos) {
    __shared__ int s_btok[256];
    __shared__ unsigned long long s_bm[TK_WORDS], s_w[TK_WORDS], s_s[TK_WORDS], s_b[TK_WORDS];
    __shared__ unsigned short s_pre[TK_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned s_first[WTILE];
    __shared__ __attribute__((aligned(16))) int s_ids[TK_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned s_pos[POS ? TK_STAGE : 4];
    const int lane = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned long long word = bm[t * TK_WORDS + (unsigned)lane];
    const unsigned wp = wpre[t * TK_WORDS + (unsigned)lane];
    const unsigned cnt = bcast_last(wp + (unsigned)__popcll(word));
    if (cnt == 0) return;                                           // (wave-uniform)
    const unsigned long long base = gpre[t / TK_GROUP] + tpre[t];
    const unsigned a = (unsigned)(base & 3ull);
    const unsigned long long tile_lo = t * WTILE;
    const unsigned long long *m = maps + t * (UG_MAPS * TK_WORDS);
    s_bm[lane] = word;
    s_w[lane] = m[lane];
    s_s[lane] = m[TK_WORDS + lane];
    s_b[lane] = m[2 * TK_WORDS + lane];
    s_pre[lane] = (unsigned short)wp;
#pragma unroll
    for (int i = 0; i < 4; i++) s_btok[i * WAVE + lane] = btok[i * WAVE + lane];
#pragma unroll
    for (int i = 0; i < WTILE / (4 * WAVE); i++)
        *reinterpret_cast<uint4 *>(&s_first[(i * WAVE + lane) * 4]) = make_uint4(~0u, ~0u, ~0u, ~0u);
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < SUBS; j++) {                                // the byte and unk tokens, in rank order
        const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
        const unsigned long long wv = s_bm[lp >> 6];
        unsigned e = (unsigned)(wv >> sh) & 0xffffu;
        if (!e) continue;
        const unsigned u = unk_id >= 0 ? (unsigned)(s_b[lp >> 6] >> sh) & 0xffffu : 0u;
        unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(sh));
        const uint4 v = tk_load16(in, tile_lo + lp, n_avail);
        const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (e >> c & 1u) {
                s_ids[rank] = (u >> c & 1u) ? unk_id : s_btok[(q[c >> 2] >> (8 * (c & 3))) & 255u];
                if constexpr (POS) s_pos[rank] = (unsigned)(tile_lo + lp + (unsigned)c);
                rank++;
            }
        }
    }
    const UgRun run = ug_run_of(tix, n_tix, cap, t);
    for (unsigned k = (unsigned)lane; k < run.cnt; k += WAVE) {     // the first record of every position
        unsigned p, s, pp = ~0u, ps;
        heap_record<BYTES>(rec, run.base + k, t, p, s);
        if (k) heap_record<BYTES>(rec, run.base + k - 1u, t, pp, ps);
        if (p != pp && (unsigned long long)p >= tile_lo && (unsigned long long)p < tile_lo + WTILE) s_first[p - (unsigned)tile_lo] = k;
    }
    wave_lds_sync();
    const bool cont0 = t > 0 && word_byte(ws, (int)in[tile_lo - 1]);
    unsigned long long pw = s_s[lane] & ~s_b[lane] & word;          // this word's piece starts
    while (pw) {
        const unsigned q = (unsigned)__builtin_ctzll(pw), lp = (unsigned)lane * 64u + q;
        pw &= pw - 1ull;
        unsigned y = (unsigned)lane;                                // the piece's end: the next bit of S | ~W
        unsigned long long cur = (s_s[y] | ~s_w[y]) & (q == 63u ? 0ull : ~0ull << (q + 1u));
        while (!cur && y < TK_WORDS + HALO_MAX / 64u) {
            y++;
            if (y < (unsigned)TK_WORDS) cur = s_s[y] | ~s_w[y];
            else if (t + 1 < n_tiles) cur = m[UG_MAPS * TK_WORDS + TK_WORDS + (y - TK_WORDS)] | ~m[UG_MAPS * TK_WORDS + (y - TK_WORDS)];
            else cur = ~0ull;
        }
        const unsigned L = cur ? y * 64u + (unsigned)__builtin_ctzll(cur) - lp : 0u;
        const bool cont = lp ? (s_w[(lp - 1u) >> 6] >> ((lp - 1u) & 63u) & 1ull) != 0ull : cont0;
        int v = PFAC_TOKEN_DROP;                                    // (no such record: not an id, so a caller would see it)
        for (unsigned k = s_first[lp]; k < run.cnt; k++) {          // the record (p, L): at most one per length
            unsigned p, s;
            heap_record<BYTES>(rec, run.base + k, t, p, s);
            if (p != (unsigned)tile_lo + lp) break;
            if (s < num_final && (unsigned)flen[s] == L) {
                const int4 pc = pieces[s];
                v = cont ? pc.y : pc.x;
                break;
            }
        }
        const unsigned long long wv = s_bm[lane];
        const unsigned rank = a + s_pre[lane] + (unsigned)__popcll(wv & tk_below(q));
        s_ids[rank] = v;
        if constexpr (POS) s_pos[rank] = (unsigned)tile_lo + lp;
    }
    wave_lds_sync();
    const unsigned long long g0 = base - a;                         // a multiple of 4: ids + g0 is 16-B aligned
    for (unsigned c = (unsigned)lane; c * 4u < a + cnt; c += WAVE) {
        const unsigned s0 = c * 4u;
        if (s0 >= a && s0 + 4u <= a + cnt) {
            *reinterpret_cast<uint4 *>(ids + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_ids[s0]);
            if constexpr (POS) *reinterpret_cast<uint4 *>(pos + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_pos[s0]);
        } else {
            for (unsigned x = s0; x < s0 + 4u; x++) {
                if (x >= a && x < a + cnt) {
                    ids[g0 + x] = s_ids[x];
                    if constexpr (POS) pos[g0 + x] = s_pos[x];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Byte-level BPE (pfac_table_set_bpe, pfac_bpe_records / _documents): the merges of every word in rank order (THE RULE
// is in pfac.h).  "Is the concatenation of these two parts a vocabulary string, and which merge makes it" is a lookup of
// (start, length) among the records of the word: the second token pass over the record heap itself, in the Unigram
// pass's structure -- a workgroup per 4 KiB tile, a region with overhang, straddling words solved by both tiles.
//   pfac_bpe_solve_kernel    a workgroup of four waves per tile.  Its region is the tile and 256 bytes on either side
//                            (the cap is at most 255: the region holds every word under the cap that touches the tile,
//                            whole).  In LDS, by region position: the bitmaps W (run bytes below n_owned), D (lead
//                            bytes), K (bytes whose byte id is kept), V (W and the lead bytes that belong to a word), P
//                            (part starts: all ones until a merge clears a boundary) and E (starts of parts of two or
//                            more bytes whose id is kept); FIRST, the index of the first record of every position in
//                            its own tile's run (one lane per record over the runs of the up to three tiles the region
//                            touches, each clipped to the region by two binary searches); and a cached candidate rank
//                            per boundary (uint32, all ones = none).  The run starts up to the tile's end are listed and
//                            dealt to the lanes, one word per lane at a time: the cache is filled for every adjacent
//                            pair of bytes, then the loop takes the first minimum of the word's boundaries (the leftmost
//                            of equal ranks), clears that bit of P and looks the two neighbouring boundaries up again.
//                            A lookup walks the records of position l in ascending length until L_s >= r - l and
//                            gathers the piece as one int4.  Words are disjoint: only the bitmap words two of them
//                            share need atomics.  At the end the lane walks its parts and sets E; one wave derives the
//                            tile's emitting positions and keeps V, P, the emit bitmap, its prefixes and the count.
//   pfac_ug_group_kernel, pfac_scan_groups_kernel, pfac_offsets_check_kernel, pfac_tk_doc_kernel: unchanged
//   pfac_bpe_docs_kernel     pfac_wp_docs_kernel with the lead rule: between a lead and its run is inside the word
//   pfac_bpe_write_kernel    pfac_ug_write_kernel's staging and stores.  Byte tokens first; then a lane per bitmap word
//                            over its starts of parts of two or more bytes: the part runs to the next bit of P | ~V (in
//                            the next tile's maps where it straddles), its id is that of the record (p, L).
constexpr int BPE_THREADS = 4 * WAVE;
constexpr int BPE_MAPS = 2;                         // V, P
constexpr int BPE_EXT = 256;                        // the region's overhang: more than the largest cap
constexpr unsigned BPE_NONE = ~0u;                  // no record / no candidate

// the highest set bit below position k (k > 0) and the lowest at or above k of an LDS bitmap of nw words
__device__ __forceinline__ unsigned bpe_prev(const volatile unsigned long long *m, unsigned k) {
    unsigned x = (k - 1u) >> 6;
    const unsigned q = (k - 1u) & 63u;
    unsigned long long v = m[x] & (q == 63u ? ~0ull : tk_below(q + 1u));
    while (!v && x > 0u) v = m[--x];
    return v ? x * 64u + 63u - (unsigned)__builtin_clzll(v) : 0u;
}
__device__ __forceinline__ unsigned bpe_next(const volatile unsigned long long *m, unsigned k, unsigned nw) {
    unsigned x = k >> 6;
    unsigned long long v = m[x] & ~tk_below(k & 63u);
    while (!v && x + 1u < nw) v = m[++x];
    return v ? x * 64u + (unsigned)__builtin_ctzll(v) : nw * 64u;
}

template <int BYTES>
__global__ void __launch_bounds__(BPE_THREADS)
pfac_bpe_solve_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tix, unsigned long long cap,
                      const unsigned char *in, unsigned long long n_avail, unsigned long long n_owned, const short *flen,
                      const int4 *pieces, const int *btok, unsigned num_final, int lead, unsigned max_word, WordSet ws,
                      unsigned long long *maps, unsigned long long *bm, unsigned short *wpre, unsigned *tcnt) {
    constexpr unsigned R = WTILE + 2 * BPE_EXT, RW = R / 64;
    __shared__ unsigned s_first[R];
    __shared__ unsigned s_rank[R];
    __shared__ unsigned short s_list[R / 2 + 64];
    __shared__ unsigned long long s_W[RW], s_D[RW], s_K[RW], s_V[RW], s_P[RW], s_E[RW];
    __shared__ unsigned long long s_rbase[3];
    __shared__ unsigned s_rcnt[3], s_rlo[3], s_rhi[3];
    __shared__ unsigned s_n;
    const unsigned tid = threadIdx.x;
    const int lane = (int)(tid & (WAVE - 1));
    const unsigned long long t = blockIdx.x;
    const unsigned long long tile_lo = t * WTILE;
    const unsigned off0 = t ? (unsigned)BPE_EXT : 0u;               // the tile's first position in the region
    const unsigned long long reg_lo = tile_lo - off0, T0 = reg_lo >> 12;
    WordSet kv;                                                     // the bytes whose byte id is kept
#pragma unroll
    for (int k = 0; k < 4; k++) kv.w[k] = __ballot(btok[k * WAVE + lane] >= 0);
    if (tid == 0) s_n = 0u;
    if (tid < 3u) {                                                 // the runs the region touches, clipped to it
        const unsigned long long tt = T0 + tid;
        const UgRun run = ug_run_of(tix, n_tix, cap, tt);
        const auto lower = [&](unsigned long long g) {              // the first record at or behind g
            unsigned lo = 0u, hi = run.cnt;
            while (lo < hi) {
                const unsigned m = lo + (hi - lo) / 2u;
                unsigned p, s;
                heap_record<BYTES>(rec, run.base + m, tt, p, s);
                if ((unsigned long long)p < g) lo = m + 1u;
                else hi = m;
            }
            return lo;
        };
        s_rbase[tid] = run.base;
        s_rcnt[tid] = run.cnt;
        s_rlo[tid] = lower(reg_lo);
        s_rhi[tid] = lower(reg_lo + R);
    }
    for (unsigned c = tid; c < R / 16; c += BPE_THREADS) {
        const unsigned long long g = reg_lo + c * 16ull;
        const unsigned dom = tk_domain16(g, 0ull, n_owned);
        unsigned wb = 0u, kb = 0u, db = 0u;
        if (dom) {
            const uint4 v = tk_load16(in, g, n_avail);
            const auto four = [&](unsigned q, int at) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int byte = (int)((q >> (8 * i)) & 255u);
                    wb |= (unsigned)word_byte(ws, byte) << (at + i);
                    kb |= (unsigned)word_byte(kv, byte) << (at + i);
                    db |= (unsigned)(byte == lead) << (at + i);
                }
            };
            four(v.x, 0);
            four(v.y, 4);
            four(v.z, 8);
            four(v.w, 12);
        }
        reinterpret_cast<unsigned short *>(s_W)[c] = (unsigned short)(wb & dom);
        reinterpret_cast<unsigned short *>(s_K)[c] = (unsigned short)(kb & dom);
        reinterpret_cast<unsigned short *>(s_D)[c] = (unsigned short)(db & dom);
    }
    for (unsigned r = tid; r < R; r += BPE_THREADS) s_first[r] = BPE_NONE;
    __syncthreads();
    for (unsigned x = tid; x < RW; x += BPE_THREADS) {
        const unsigned long long W = s_W[x];
        // a start: a run byte with none in front of it; what lies in front of the region is not known (taken as one)
        const unsigned long long top = x ? s_W[x - 1] >> 63 : (reg_lo ? 1ull : 0ull);
        unsigned long long st = W & ~(W << 1 | top);
        const unsigned long long nst0 = x + 1u < RW ? s_W[x + 1] & 1ull & ~(W >> 63) : 0ull;
        s_V[x] = W | (((st >> 1) | (nst0 << 63)) & s_D[x]);         // the lead byte in front of a start belongs to its word
        s_P[x] = ~0ull;
        s_E[x] = 0ull;
        // the words that start behind the tile are not its own; a run that starts right behind it may have its lead inside
        if (x * 64u > off0 + WTILE) st = 0ull;
        else if (x * 64u == off0 + WTILE) st &= 1ull;
        while (st) {
            const unsigned b = (unsigned)__builtin_ctzll(st);
            st &= st - 1ull;
            s_list[atomicAdd(&s_n, 1u)] = (unsigned short)(x * 64u + b);
        }
    }
    for (unsigned ti = 0; ti < 3u; ti++) {                          // the first record of every region position
        const unsigned long long tt = T0 + ti, base = s_rbase[ti];
        const unsigned hi = s_rhi[ti];
        for (unsigned k = s_rlo[ti] + tid; k < hi; k += BPE_THREADS) {
            unsigned p, s, pp = ~0u, ps;
            heap_record<BYTES>(rec, base + k, tt, p, s);
            if (k) heap_record<BYTES>(rec, base + k - 1u, tt, pp, ps);
            const unsigned long long rp = (unsigned long long)p - reg_lo;
            if (p != pp && rp < R) s_first[(unsigned)rp] = k;
        }
    }
    __syncthreads();
    // the state of the record (l, len), or BPE_NONE: the records of a position ascend in length
    const auto find = [&](unsigned l, unsigned len) -> unsigned {
        unsigned k = s_first[l];
        if (k == BPE_NONE) return BPE_NONE;
        const unsigned long long gl = reg_lo + l, tt = gl >> 12;
        const unsigned ti = (unsigned)(tt - T0);
        const unsigned long long base = s_rbase[ti];
        const unsigned cnt = s_rcnt[ti];
        for (; k < cnt; k++) {
            unsigned p, s;
            heap_record<BYTES>(rec, base + k, tt, p, s);
            if ((unsigned long long)p != gl) break;
            if (s >= num_final) continue;
            const int L = flen[s];
            if (L < (int)len) continue;
            return L == (int)len ? s : BPE_NONE;
        }
        return BPE_NONE;
    };
    // the rank of the candidate [l, k) + [k, r), or BPE_NONE
    const auto cand = [&](unsigned l, unsigned k, unsigned r) -> unsigned {
        const unsigned s = find(l, r - l);
        if (s == BPE_NONE) return BPE_NONE;
        const int4 pc = pieces[s];
        return (pc.z == 0 || (unsigned)pc.z == k - l) ? (unsigned)pc.y : BPE_NONE;
    };
    const unsigned n_words = s_n;
    for (unsigned w = tid; w < n_words; w += BPE_THREADS) {
        const unsigned a0 = s_list[w];
        unsigned b = R;                                             // the run's end: the first 0 of W behind a0
        {
            unsigned x = a0 >> 6;
            unsigned long long inv = ~s_W[x] & ~tk_below(a0 & 63u);
            while (!inv && x + 1u < RW && (x + 1u) * 64u <= a0 + max_word) inv = ~s_W[++x];
            if (inv) b = x * 64u + (unsigned)__builtin_ctzll(inv);
        }
        const unsigned a = a0 > 0u && (s_D[(a0 - 1u) >> 6] >> ((a0 - 1u) & 63u) & 1ull) ? a0 - 1u : a0;
        // over the cap (single bytes, as P stands), in front of the tile, behind it, or one byte: nothing to merge
        if (b - a > max_word || b <= off0 || a >= off0 + WTILE || b - a < 2u) continue;
        for (unsigned k = a + 1u; k < b; k++) s_rank[k] = cand(k - 1u, k, k + 1u);
        for (;;) {
            unsigned best = BPE_NONE, at = 0u;
            for (unsigned k = a + 1u; k < b; k++) {
                const unsigned r = s_rank[k];
                if (r < best) {
                    best = r;
                    at = k;
                }
            }
            if (best == BPE_NONE) break;
            atomicAnd(&s_P[at >> 6], ~(1ull << (at & 63u)));
            s_rank[at] = BPE_NONE;
            const unsigned l = bpe_prev(s_P, at), r = bpe_next(s_P, at + 1u, RW);
            if (l > a) s_rank[l] = cand(bpe_prev(s_P, l), l, r);
            if (r < b) s_rank[r] = cand(l, r, bpe_next(s_P, r + 1u, RW));
        }
        for (unsigned l = a; l < b;) {                              // the parts of two or more bytes whose id is kept
            const unsigned r = bpe_next(s_P, l + 1u, RW);
            if (r - l >= 2u) {
                const unsigned s = find(l, r - l);
                if (s != BPE_NONE && pieces[s].x >= 0) atomicOr(&s_E[l >> 6], 1ull << (l & 63u));
            }
            l = r;
        }
    }
    __syncthreads();
    if (tid < WAVE) {
        const unsigned x = off0 / 64u + (unsigned)lane;
        const unsigned long long V = s_V[x], P = s_P[x], K = s_K[x], E = s_E[x];
        const unsigned long long Vn = V >> 1 | s_V[x + 1] << 63, Pn = P >> 1 | s_P[x + 1] << 63;
        const unsigned long long multi = V & P & Vn & ~Pn;          // a part start with a byte of its part behind it
        const unsigned long long word = (~(V & ~P) & ~multi & K) | (multi & E);
        const unsigned c = (unsigned)__popcll(word), incl = wave_incl_scan(c);
        unsigned long long *m = maps + t * (BPE_MAPS * TK_WORDS);
        m[lane] = V;
        m[TK_WORDS + lane] = P;
        bm[t * TK_WORDS + (unsigned)lane] = word;
        wpre[t * TK_WORDS + (unsigned)lane] = (unsigned short)(incl - c);
        if (lane == WAVE - 1) tcnt[t] = incl;
    }
}

// every document offset outside every word (three byte loads per offset, all below n_owned): between two run bytes, or
// between a lead byte and the run behind it, is inside; else bit 1 of *err
__global__ void pfac_bpe_docs_kernel(const unsigned long long *off, unsigned long long n_docs, unsigned long long n_owned,
                                     const unsigned char *in, WordSet ws, int lead, unsigned long long *err) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    bool bad = false;
    for (unsigned long long d = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
        const unsigned long long o = off[d];
        if (o > 0 && o < n_owned) {
            const int front = (int)in[o - 1];
            bad |= word_byte(ws, (int)in[o]) && (word_byte(ws, front) || front == lead);
        }
    }
    if (bad) atomicOr(err, 2ull);
}

template <int BYTES, bool POS>
__global__ void __launch_bounds__(WAVE)
pfac_bpe_write_kernel(const void *rec, const unsigned long long *tix, unsigned long long n_tix, unsigned long long cap,
                      const unsigned char *in, unsigned long long n_avail, const short *flen, const int4 *pieces,
                      const int *btok, unsigned num_final, const unsigned long long *maps, unsigned long long n_tiles,
                      const unsigned long long *bm, const unsigned short *wpre, const unsigned *tpre,
                      const unsigned long long *gpre, int *ids, unsigned *pos) {
    __shared__ int s_btok[256];
    __shared__ unsigned long long s_bm[TK_WORDS], s_v[TK_WORDS], s_p[TK_WORDS];
    __shared__ unsigned short s_pre[TK_WORDS];
    __shared__ __attribute__((aligned(16))) unsigned s_first[WTILE];
    __shared__ __attribute__((aligned(16))) int s_ids[TK_STAGE];
    __shared__ __attribute__((aligned(16))) unsigned s_pos[POS ? TK_STAGE : 4];
    const int lane = threadIdx.x;
    const unsigned long long t = blockIdx.x;
    const unsigned long long word = bm[t * TK_WORDS + (unsigned)lane];
    const unsigned wp = wpre[t * TK_WORDS + (unsigned)lane];
    const unsigned cnt = bcast_last(wp + (unsigned)__popcll(word));
    if (cnt == 0) return;                                           // (wave-uniform)
    const unsigned long long base = gpre[t / TK_GROUP] + tpre[t];
    const unsigned a = (unsigned)(base & 3ull);
    const unsigned long long tile_lo = t * WTILE;
    const unsigned long long *m = maps + t * (BPE_MAPS * TK_WORDS), *mn = m + BPE_MAPS * TK_WORDS;
    const bool more = t + 1 < n_tiles;                              // (else mn is not there)
    s_bm[lane] = word;
    s_v[lane] = m[lane];
    s_p[lane] = m[TK_WORDS + lane];
    s_pre[lane] = (unsigned short)wp;
#pragma unroll
    for (int i = 0; i < 4; i++) s_btok[i * WAVE + lane] = btok[i * WAVE + lane];
#pragma unroll
    for (int i = 0; i < WTILE / (4 * WAVE); i++)
        *reinterpret_cast<uint4 *>(&s_first[(i * WAVE + lane) * 4]) = make_uint4(~0u, ~0u, ~0u, ~0u);
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < SUBS; j++) {                                // the byte tokens, in rank order (a part start's is replaced below)
        const unsigned lp = (unsigned)j * SUB + (unsigned)lane * 16u, sh = lp & 63u;
        const unsigned long long wv = s_bm[lp >> 6];
        const unsigned e = (unsigned)(wv >> sh) & 0xffffu;
        if (!e) continue;
        unsigned rank = a + s_pre[lp >> 6] + (unsigned)__popcll(wv & tk_below(sh));
        const uint4 v = tk_load16(in, tile_lo + lp, n_avail);
        const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (e >> c & 1u) {
                s_ids[rank] = s_btok[(q[c >> 2] >> (8 * (c & 3))) & 255u];
                if constexpr (POS) s_pos[rank] = (unsigned)(tile_lo + lp + (unsigned)c);
                rank++;
            }
        }
    }
    const UgRun run = ug_run_of(tix, n_tix, cap, t);
    for (unsigned k = (unsigned)lane; k < run.cnt; k += WAVE) {     // the first record of every position
        unsigned p, s, pp = ~0u, ps;
        heap_record<BYTES>(rec, run.base + k, t, p, s);
        if (k) heap_record<BYTES>(rec, run.base + k - 1u, t, pp, ps);
        if (p != pp && (unsigned long long)p >= tile_lo && (unsigned long long)p < tile_lo + WTILE) s_first[p - (unsigned)tile_lo] = k;
    }
    wave_lds_sync();
    const unsigned long long V = s_v[lane], P = s_p[lane];
    const unsigned long long nV = lane + 1 < TK_WORDS ? s_v[lane + 1] : (more ? mn[0] : 0ull);
    const unsigned long long nP = lane + 1 < TK_WORDS ? s_p[lane + 1] : (more ? mn[TK_WORDS] : ~0ull);
    unsigned long long pw = V & P & (V >> 1 | nV << 63) & ~(P >> 1 | nP << 63) & word;    // this word's starts of parts of >= 2 bytes
    while (pw) {
        const unsigned q = (unsigned)__builtin_ctzll(pw), lp = (unsigned)lane * 64u + q;
        pw &= pw - 1ull;
        unsigned y = (unsigned)lane;                                // the part's end: the next bit of P | ~V
        unsigned long long cur = (s_p[y] | ~s_v[y]) & (q == 63u ? 0ull : ~0ull << (q + 1u));
        while (!cur && y < TK_WORDS + BPE_EXT / 64u) {
            y++;
            if (y < (unsigned)TK_WORDS) cur = s_p[y] | ~s_v[y];
            else if (more) cur = mn[TK_WORDS + (y - TK_WORDS)] | ~mn[y - TK_WORDS];
            else cur = ~0ull;
        }
        const unsigned L = cur ? y * 64u + (unsigned)__builtin_ctzll(cur) - lp : 0u;
        int v = PFAC_TOKEN_DROP;                                    // (no such record: not an id, so a caller would see it)
        for (unsigned k = s_first[lp]; k < run.cnt; k++) {          // the record (p, L): at most one per length
            unsigned p, s;
            heap_record<BYTES>(rec, run.base + k, t, p, s);
            if (p != (unsigned)tile_lo + lp) break;
            if (s < num_final && (unsigned)flen[s] == L) {
                v = pieces[s].x;
                break;
            }
        }
        const unsigned rank = a + s_pre[lane] + (unsigned)__popcll(word & tk_below(q));
        s_ids[rank] = v;
        if constexpr (POS) s_pos[rank] = (unsigned)tile_lo + lp;
    }
    wave_lds_sync();
    const unsigned long long g0 = base - a;                         // a multiple of 4: ids + g0 is 16-B aligned
    for (unsigned c = (unsigned)lane; c * 4u < a + cnt; c += WAVE) {
        const unsigned s0 = c * 4u;
        if (s0 >= a && s0 + 4u <= a + cnt) {
            *reinterpret_cast<uint4 *>(ids + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_ids[s0]);
            if constexpr (POS) *reinterpret_cast<uint4 *>(pos + g0 + s0) = *reinterpret_cast<const uint4 *>(&s_pos[s0]);
        } else {
            for (unsigned x = s0; x < s0 + 4u; x++) {
                if (x >= a && x < a + cnt) {
                    ids[g0 + x] = s_ids[x];
                    if constexpr (POS) pos[g0 + x] = s_pos[x];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Proximity rules (pfac_documents_near): bit r of mask[d] is set iff document d holds two distinct records i < j, at
// most max_dist bytes apart by their starts, that are an (A_r, B_r) pair -- in either order unless the rule is ordered.
// With a maximum distance only, the nearest earlier A (or B) is the best partner a record can have, so the pass needs
// per record and rule "the last A / the last B in front of me" and nothing else: O(N x n_rules) whatever max_dist is.
// The records of a document are contiguous and ordered, so that partner comes from ballots, not from a scan over values.
// NR_BLOCK records per wave, 64 per chunk; three kernels:
//   pfac_near_last_kernel    one wave per block: per (rule, side) the index and position of the block's last A / last B
//                            (NR_NONE: none), into tab[(2 r + side) * n_blocks + block].  The chunks are walked from the
//                            block's end and only for the rules still open, so a rule whose classes are common costs one
//                            chunk.  Lane r keeps rule r's two answers.
//   pfac_near_carry_kernel   one workgroup per (rule, side): its row becomes, in place, the exclusive "last entry that is
//                            not NR_NONE" over the blocks -- each block's carry-in -- 256 blocks per trip.
//   pfac_near_kernel         the pass: one read of the records.  Per chunk a lane loads its record, gathers
//                            groups[state] and finds its document by the bounded searches of pfac_sel_scores_kernel.
//                            Per rule two ballots; a lane's last earlier A in the chunk is the top bit of the ballot
//                            below the lane, its position one lane permute; with no earlier A in the chunk the partner
//                            is the rule's carry (index, position).  A wave cannot keep 64 x 2 carries in scalar
//                            registers: LANE r holds rule r's, read with a readlane at the loop's (uniform) rule index
//                            and moved on from the ballot's top bit.  The lane fires iff the partner's index is at or
//                            above doc_first[d] and the distance is within max_dist.  The fired bits of a lane are one
//                            word; the per-document OR is doc_reduce_chunk<GroupOr>, with the store rule of
//                            pfac_sel_scores_kernel: a document inside the wave's block is stored plainly over the
//                            memset's 0, the at most two that straddle its ends are ORed atomically.
// Checked in the pass, into res[1]: first[0] == 0, no decrease, first[n_docs] == n, every state below num_final, no
// position that decreases inside a document.  Behind a failed check the masks are garbage in bounds and the host
// discards them.  A state past the table reads no group (in all three kernels).
constexpr unsigned NR_BLOCK = 64 * WAVE;
#define GRID_THREAD ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x)        // (as the document kernels define them)
#define GRID_THREADS ((unsigned long long)gridDim.x * blockDim.x)
constexpr unsigned long long NR_NONE = ~0ull;                       // (index | position << 32; an index stays below 2^32 - 1)
static_assert(sizeof(pfac_near_rule) == 32, "a rule is two dwordx4");

__device__ __forceinline__ unsigned long long nr_or64(unsigned long long v) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) v |= __shfl_xor(v, s, WAVE);
    return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32 |
           (unsigned)__builtin_amdgcn_readfirstlane((int)v);     // (uniform, and known to be)
}

__global__ void __launch_bounds__(256)
pfac_near_last_kernel(const pfac_record *sel, unsigned long long n, const unsigned long long *gmask, unsigned num_final,
                      const pfac_near_rule *__restrict__ rules, unsigned n_rules, unsigned n_blocks, unsigned long long *tab) {
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned blk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (blk >= n_blocks) return;                                // (wave-uniform)
    const unsigned long long p0 = (unsigned long long)blk * NR_BLOCK, p1 = min(p0 + NR_BLOCK, n);
    unsigned long long open[2];                                 // the rules without an answer yet, per side (uniform)
    open[0] = open[1] = n_rules >= 64u ? ~0ull : (1ull << n_rules) - 1ull;
    unsigned long long last[2] = {NR_NONE, NR_NONE};            // lane r: rule r's last A, last B
    const unsigned n_chunks = (unsigned)((p1 - p0 + WAVE - 1) / WAVE);
    for (unsigned c = n_chunks; c-- > 0 && (open[0] | open[1]) != 0ull;) {
        const unsigned long long c0 = p0 + (unsigned long long)c * WAVE, i = c0 + (unsigned)lane;
        const bool have = i < p1;
        pfac_record rec;
        rec.pos = 0u;
        rec.state = 0u;
        if (have) rec = sel[i];
        const unsigned long long g = have && rec.state < num_final ? gmask[rec.state] : 0ull;
        const unsigned long long any = nr_or64(g);
#pragma unroll
        for (int side = 0; side < 2; side++) {
            for (unsigned long long todo = open[side]; todo != 0ull; todo &= todo - 1ull) {
                const int r = __ffsll((long long)todo) - 1;
                const unsigned long long want = side ? rules[r].b_groups : rules[r].a_groups;
                if (want == 0ull) { open[side] &= ~(1ull << r); continue; }       // it never matches: NR_NONE stands
                if ((any & want) == 0ull) continue;
                const unsigned long long bal = __ballot((g & want) != 0ull);
                const int top = 63 - __clzll((long long)bal);
                const unsigned tpos = (unsigned)__builtin_amdgcn_readlane((int)rec.pos, top);
                if (lane == r) last[side] = (c0 + (unsigned)top) | (unsigned long long)tpos << 32;
                open[side] &= ~(1ull << r);
            }
        }
    }
    if ((unsigned)lane < n_rules) {
        tab[(unsigned long long)(2 * lane) * n_blocks + blk] = last[0];
        tab[(unsigned long long)(2 * lane + 1) * n_blocks + blk] = last[1];
    }
}

__global__ void __launch_bounds__(256)
pfac_near_carry_kernel(unsigned long long *tab, unsigned n_blocks) {
    __shared__ unsigned long long wlast[4];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    unsigned long long *row = tab + (unsigned long long)blockIdx.x * n_blocks;
    unsigned long long carry = NR_NONE;
    for (unsigned b0 = 0; b0 < n_blocks; b0 += 256) {
        const unsigned b = b0 + threadIdx.x;
        const unsigned long long v = b < n_blocks ? row[b] : NR_NONE;
        unsigned long long inc = v;                             // the last entry at or below this lane, inside the wave
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) {
            const unsigned long long u = __shfl_up(inc, s, WAVE);
            if (lane >= s && inc == NR_NONE) inc = u;
        }
        __syncthreads();                                        // (the trip before has read wlast)
        if (lane == WAVE - 1) wlast[wave] = inc;
        __syncthreads();
        unsigned long long pre = carry;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const unsigned long long w = wlast[j];
            if (w != NR_NONE) {
                if (j < wave) pre = w;
                carry = w;
            }
        }
        unsigned long long ex = __shfl_up(inc, 1, WAVE);
        if (lane == 0 || ex == NR_NONE) ex = pre;
        if (b < n_blocks) row[b] = ex;
    }
}

// the partner of a lane among the other side's records: the last one below the lane in this chunk (ballot `other`), else
// the rule's carry (ci, cp); fires iff there is one inside the lane's document and within max_dist
__device__ __forceinline__ bool nr_fires(bool mine, unsigned long long other, unsigned long long below, unsigned c0, unsigned pos,
                                         unsigned dstart, unsigned ci, unsigned cp, unsigned max_dist) {
    const unsigned long long m = other & below;
    const int src = m ? 63 - __clzll((long long)m) : 0;
    const unsigned ppos = (unsigned)__shfl((int)pos, src, WAVE);
    const unsigned idx = m ? c0 + (unsigned)src : ci, at = m ? ppos : cp;
    const bool any = m != 0ull || ci != 0xFFFFFFFFu;
    return mine && any && idx >= dstart && pos - at <= max_dist;
}

__global__ void __launch_bounds__(256)
pfac_near_kernel(const pfac_record *sel, unsigned long long n, const unsigned long long *first, unsigned long long n_docs,
                 const unsigned long long *gmask, unsigned num_final, const pfac_near_rule *__restrict__ rules, unsigned n_rules,
                 unsigned n_blocks, const unsigned long long *tab, unsigned long long *out, unsigned long long *res) {
    using R = GroupOr;
    bool bad = false;
    for (unsigned long long d = GRID_THREAD; d < n_docs; d += GRID_THREADS) bad = bad || first[d] > first[d + 1];
    if (GRID_THREAD == 0) bad = bad || first[0] != 0ull || first[n_docs] != n;
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned blk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (blk < n_blocks && n_docs) {                             // (wave-uniform)
        const unsigned long long p0 = (unsigned long long)blk * NR_BLOCK, p1 = min(p0 + NR_BLOCK, n);
        const unsigned long long ia = doc_lower_bound(first, n_docs + 1, p0);
        const unsigned long long ib = p1 >= n ? n_docs + 1 : doc_lower_bound(first, n_docs + 1, p1 + 1ull);
        const unsigned long long ie = ib ? ib - 1 : 0ull;
        auto flush = [&](unsigned d, R::Val m) {
            if (R::empty(m)) return;
            if (d >= ia && d < ie) R::store(out, d, m);
            else R::atomic(out, d, m);
        };
        // lane r: the carries of rule r (the last A and the last B in front of the chunk)
        unsigned long long ca = NR_NONE, cb = NR_NONE;
        if ((unsigned)lane < n_rules) {
            ca = tab[(unsigned long long)(2 * lane) * n_blocks + blk];
            cb = tab[(unsigned long long)(2 * lane + 1) * n_blocks + blk];
        }
        unsigned cai = (unsigned)ca, cap = (unsigned)(ca >> 32), cbi = (unsigned)cb, cbp = (unsigned)(cb >> 32);
        const unsigned long long below = (1ull << lane) - 1ull;
        bool cvalid = false;
        unsigned cd = 0;
        R::Val cm = R::none(), any = R::none();
        unsigned long long dlo = doc_of(first, 0ull, n_docs - 1, p0);
        const unsigned long long dtop = doc_of(first, dlo, n_docs - 1, p1 - 1);
        unsigned lastpos = p0 ? sel[p0 - 1].pos : 0u;            // the position in front of the chunk (uniform)
        for (unsigned long long c0 = p0; c0 < p1; c0 += WAVE) {
            const unsigned long long i = c0 + (unsigned)lane;
            const bool have = i < p1;
            pfac_record rec;
            rec.pos = 0u;
            rec.state = 0u;
            if (have) rec = sel[i];
            const bool known = rec.state < num_final;
            bad = bad || !known;
            const unsigned long long g = have && known ? gmask[rec.state] : 0ull;
            dlo = doc_of(first, dlo, dtop, c0);
            const unsigned long long dhi = doc_of(first, dlo, dtop, min(c0 + (WAVE - 1), p1 - 1));
            const unsigned long long d = have ? doc_of(first, dlo, dhi, i) : dlo;
            const unsigned dstart = (unsigned)first[d];
            const unsigned pos = rec.pos;
            unsigned prev = (unsigned)__shfl_up((int)pos, 1, WAVE);
            if (lane == 0) prev = lastpos;
            bad = bad || (have && (unsigned)i > dstart && pos < prev);
            lastpos = (unsigned)__builtin_amdgcn_readlane((int)pos, WAVE - 1);
            unsigned long long fired = 0ull;
            for (unsigned r = 0; r < n_rules; r++) {
                const unsigned long long ag = rules[r].a_groups, bg = rules[r].b_groups;
                const unsigned max_dist = rules[r].max_dist;
                const bool both = !(rules[r].flags & PFAC_NEAR_ORDERED);
                const bool isa = (g & ag) != 0ull, isb = (g & bg) != 0ull;
                const unsigned long long ba = __ballot(isa), bb = __ballot(isb);
                if ((ba | bb) == 0ull) continue;                // (uniform) neither class in this chunk: the carries stand
                const unsigned rai = (unsigned)__builtin_amdgcn_readlane((int)cai, (int)r);
                const unsigned rap = (unsigned)__builtin_amdgcn_readlane((int)cap, (int)r);
                bool fire = false;
                if (bb != 0ull) fire = nr_fires(isb, ba, below, (unsigned)c0, pos, dstart, rai, rap, max_dist);
                if (both && ba != 0ull) {
                    const unsigned rbi = (unsigned)__builtin_amdgcn_readlane((int)cbi, (int)r);
                    const unsigned rbp = (unsigned)__builtin_amdgcn_readlane((int)cbp, (int)r);
                    fire = nr_fires(isa, bb, below, (unsigned)c0, pos, dstart, rbi, rbp, max_dist) || fire;
                }
                if (fire) fired |= 1ull << r;
                if (ba != 0ull) {
                    const int top = 63 - __clzll((long long)ba);
                    const unsigned tpos = (unsigned)__builtin_amdgcn_readlane((int)pos, top);
                    if ((unsigned)lane == r) { cai = (unsigned)c0 + (unsigned)top; cap = tpos; }
                }
                if (bb != 0ull) {
                    const int top = 63 - __clzll((long long)bb);
                    const unsigned tpos = (unsigned)__builtin_amdgcn_readlane((int)pos, top);
                    if ((unsigned)lane == r) { cbi = (unsigned)c0 + (unsigned)top; cbp = tpos; }
                }
            }
            const unsigned long long b = __ballot(fired != 0ull);
            if (b == 0ull) continue;
            R::add(any, fired);
            doc_reduce_chunk<R>(lane, b, d, fired, cvalid, cd, cm, flush);
        }
        if (cvalid && lane == 0) flush(cd, cm);
        R::total(res, any, lane);
    }
    if (bad) res[1] = 1ull;
}
#undef GRID_THREAD
#undef GRID_THREADS

// ---------------------------------------------------------------------------
// runtime

thread_local std::string g_err;

int fail(pfac_ctx *ctx, int code, const std::string &msg);

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, PFAC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// A device allocation that a context or a slot owns: pointer and capacity (in elements of T) live and die together.
// It only grows, and the caller names the new capacity -- the growth policies differ per buffer on purpose.  The
// lifetime rule of the runtime is kept HERE: nothing queued on the owner's stream may still use the buffer when it
// is freed, so a slot's buffer is grown with the slot's stream, which is synchronised first (the context's table
// buffers and a call's temporaries pass none: install_table waits for the scans in flight itself).  Freed with its
// owner: pfac_ctx_destroy synchronises the streams, then deletes the context under its device guard.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    uint64_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    int ensure(pfac_ctx *ctx, hipStream_t stream, uint64_t need, uint64_t new_cap) {
        if (need <= cap) return PFAC_OK;
        if (p) {
            if (stream) HIP_TRY(ctx, hipStreamSynchronize(stream));
            HIP_TRY(ctx, hipFree(p));
            p = nullptr;
            cap = 0;
        }
        HIP_TRY(ctx, hipMalloc((void **)&p, new_cap * sizeof(T)));
        cap = new_cap;
        return PFAC_OK;
    }
};

// An output of a pass that goes to the caller's device buffer or to this slot-owned one, and what ties the buffer to
// its result: n elements, `done` (the pass has finished since it last invalidated), `own` (it wrote here, not into the
// caller's buffer).  The rule it owns: a pass invalidates its outputs before its first check -- a refused call discards
// the slot's earlier result -- and commits them together, behind its last launch.  Only a done, own result is fetched
// (fetch) or stands in for a NULL argument of the pass that follows (consume).
constexpr uint64_t ANY_N = ~0ull;         // consume: the caller names no count
template <typename T>
struct PassOut {
    DevBuf<T> buf;
    uint64_t n = 0;
    bool done = false, own = false;
    void invalidate() { done = false; }
    void commit(uint64_t n_, bool own_) { n = n_; own = own_; done = true; }
    // where `need` elements go: the caller's buffer, or the slot's grown (with the slot's stream) to the capacity the pass names
    template <typename U>
    int bind(pfac_ctx *ctx, hipStream_t stream, U *caller, uint64_t need, uint64_t new_cap, T **dst) {
        int rc = caller ? PFAC_OK : buf.ensure(ctx, stream, need, new_cap);
        *dst = caller ? reinterpret_cast<T *>(caller) : buf.p;
        return rc;
    }
    // the NULL default of the next pass's argument: the caller's pointer, or this result where it is the slot's
    template <typename U>
    int consume(pfac_ctx *ctx, const std::string &fn, const char *noun, const U *caller, uint64_t expect, const T **src) const {
        *src = reinterpret_cast<const T *>(caller);
        if (caller) return PFAC_OK;
        if (!done || !own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no " + noun + " (none yet, or it went to the caller's buffer; pass that)");
        if (expect != ANY_N && expect != n) return fail(ctx, PFAC_E_ARG, fn + ": the count given differs from the slot's " + noun);
        *src = buf.p;
        return PFAC_OK;
    }
};

// capacity of a per-tile array asked for n entries: a quarter more, 4096 at least
uint64_t quarter_more(uint64_t n) { return n < 4096 ? 4096 : n + n / 4; }
// ... of a slot-owned array of n_docs + 1 entries (offsets, doc_first)
uint64_t docs_cap(uint64_t n_docs) { return n_docs + 1 < 4096 ? 4096 : n_docs + 1 + n_docs / 4; }

// 64-bit words in Slot::h_ctl (as indices of its 32-bit words)
enum : int {
    H_MATCHES = 0,                        // written by the scan kernel: matches, ...
    H_USED = 4,                           // ... heap records used
    H_DONE = RES_DONE,                    // (one 32-bit word) the scan's completion: cleared by pfac_scan_async, set by the kernel
    H_CHECKSUM = 8,                       // pfac_records_checksum
    H_PASS = 10,                          // what a pass copies back from behind its group prefixes: the total, ...
    H_PASS1 = 12,                         // ... the word behind it (segment: bad offsets; selection: exit offset; replace: error), ...
    H_PASS2 = 14,                         // ... and the one behind that (document selection: bad offsets; replace: c_{n-1})
    H_T0 = RES_T0, H_T1 = RES_T1,         // written by the scan kernel: its start and end by its own clock (ticks)
    H_CTL_BYTES = 128,
};

struct Slot {
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DevBuf<unsigned char> input;
    DevBuf<pfac_record> records;          // cap x 8 bytes: holds either record format
    DevBuf<unsigned long long> tile_index;        // per tile of the last scan: first record | count << 40
    DevBuf<unsigned> d2log;               // dense mode, second form: the record logs of the grid's compute waves
    DevBuf<unsigned long long> gsum;      // scratch of the expand / text paths: record (byte) prefix per group of 64 tiles (+ the total)
    DevBuf<unsigned char> text;           // pfac_emit_text_device: the formatted lines of the slot's last scan (no PassOut:
    uint64_t text_bytes = 0;              // it has no "never made" state -- before the first text its length is 0)
    DevBuf<pfac_record> wide;             // scratch of pfac_records_d2h: packed records expanded on the device
    int last_rec_bytes = 4;               // record form of the slot's last scan (2, 4 or 8 bytes)
    const void *last_records = nullptr;   // ... and where it wrote
    DevBuf<unsigned> ctl;                 // TWO control headers (ticket counters, flags, heap cursor), used alternately:
    unsigned *d_ctlbuf[2] = {nullptr, nullptr};   // a scan zeroes the other one for the scan after it
    bool clean[2] = {false, false};       // header known to be zero
    int flip = 0;                         // header of the next scan
    unsigned *h_ctl = nullptr;            // pinned, device-visible: [0..1] matches, [2] err, [3] dense tiles, [4..5] heap
                                          // records used, [7] done, [16..19] start and end time (written by the kernel),
                                          // [8..9] checksum, [10..15] a pass's results (the H_ constants above name them)
    unsigned *d_res = nullptr;            // device-side address of h_ctl
    DevBuf<unsigned long long> sum;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;      // PFAC_EVENT_TIMING only (else null): start / stop events on the scan's dispatch
    double spin_ms = 0;                   // how long wait_scan polls for the pending scan before it asks the stream
    hipEvent_t ev_h2d = nullptr;          // behind the slot's last pfac_slot_h2d: the host buffer may be reused once it has fired
    hipEvent_t ev_rd = nullptr;           // recorded on the slot's stream at a pfac_slot_h2d: behind every queued reader of the input
    bool h2d_issued = false;
    uint64_t last_cap = 0, last_tiles = 0, last_total = 0, last_used = 0;
    bool scanned = false, pending = false, last_dense = false;
    uint64_t last_owned = 0;              // n_owned of the slot's last scan (what pfac_records_segment cuts)
    uint64_t last_table = 0;              // ... and the table it ran with (pfac_ctx::table_gen)
    DevBuf<unsigned long long> dbg;       // PFAC_TRACE_BUILD + PFAC_TRACE
    // pfac_slot_doc_offsets / pfac_records_segment
    PassOut<unsigned long long> doc;      // the slot's document offsets (n_docs + 1 of them; always the slot's own)
    DevBuf<unsigned> seg_tcnt;            // kept records per tile of the last segment pass
    PassOut<pfac_record> seg_out;         // the last segment pass: the kept records, ...
    PassOut<unsigned long long> seg_first;        // ... and doc_first (n_docs + 1 entries)
    // pfac_records_leftmost_longest
    DevBuf<unsigned char> ll_tmp;         // group functions, group entries, picks per tile, per-tile selection bitmaps
    PassOut<pfac_record> ll_out;          // the selection
    uint64_t ll_seq = 0;                  // the scan it selected from (scan_seq), ...
    uint32_t ll_entry = 0, ll_exit = 0;   // ... and its entry and exit offsets
    // pfac_replace_leftmost_longest
    uint64_t last_avail = 0;              // n_avail of the slot's last scan (the input bytes it may read)
    uint64_t scan_seq = 0;                // record sets of this slot: scans issued + whole-word filters run over them
    DevBuf<unsigned char> rp_tmp;         // X per block of 64 picks
    PassOut<unsigned char> rp_out;        // the output bytes
    // pfac_extract_leftmost_longest (X and the group prefixes are the replace's scratch: both are used up on the stream)
    PassOut<unsigned char> ex_out;        // the rewritten picks, back to back, ...
    PassOut<unsigned long long> ex_off;   // ... and their output offsets (n + 1 entries)
    // pfac_records_leftmost_longest_documents / pfac_replace_documents
    uint64_t doc_gen = 0;                 // pfac_slot_doc_offsets calls: a selection remembers the offsets it cut with
    bool ll_docs = false;                 // the slot's last selection was per document, ...
    uint64_t lld_gen = 0;                 // ... with the slot's offsets of this generation
    bool lld_own_off = false;             // (or the caller's offsets)
    PassOut<unsigned long long> lld_first;        // its doc_first (n_docs + 1 entries)
    DevBuf<unsigned long long> rpd_tmp;   // D_k per pick (and the total behind them)
    PassOut<unsigned long long> rpd_off;  // the output offsets (n_docs + 1 entries)
    // pfac_records_count_states / pfac_selection_count_states
    PassOut<unsigned long long> cnt;      // the state counts; committed by slot-owned counts only, never invalidated: they
    uint64_t cnt_table = 0;               // accumulate across calls.  Counted with this table (pfac_ctx::table_gen)
    // pfac_slot_doc_offsets_split
    DevBuf<unsigned long long> sp_tile;   // per input tile: delimiters | end of the last one << 32
    // pfac_documents_matching
    PassOut<unsigned long long> dm_out;   // the ids
    // pfac_documents_group_masks
    PassOut<unsigned long long> gm_out;   // the masks (n_docs of them); scratch of a call that writes to the caller's buffer
    // pfac_documents_scores / pfac_selection_document_scores
    PassOut<pfac_doc_score> sc_out;       // the scores (n_docs of them); scratch of a call that writes to the caller's buffer
    // pfac_documents_top_scores (its ids are dm_out)
    DevBuf<unsigned long long> tp_work;   // the select's histograms and its state words
    DevBuf<ulonglong2> tp_ent;            // PFAC_TOP_RANKED: the sort's two buffers of (key word, id), n_top entries each, ...
    DevBuf<unsigned long long> tp_bh;     // ... and its digit counts per block (and the total behind them)
    PassOut<pfac_doc_score> tp_out;       // the winners' pairs
    // pfac_documents_term_counts
    uint64_t seg_table = 0;               // the table the slot's last segment pass ran with (pfac_ctx::table_gen)
    DevBuf<unsigned long long> tc_keys;   // the sort's two buffers of keys, n entries each, ...
    DevBuf<unsigned> tc_bh;               // ... its digit counts per workgroup (and the 256 digit sums behind them), ...
    DevBuf<unsigned long long> tc_bal;    // ... the head ballot of every block of 64 sorted keys, ...
    DevBuf<unsigned> tc_x;                // ... the heads in front of the block in its group, ...
    DevBuf<unsigned> tc_hidx;             // ... and the index of every head (n_terms + 1 entries)
    PassOut<unsigned long long> tc_row;   // row_ptr (n_docs + 1 entries), ...
    PassOut<unsigned> tc_st, tc_cnt;      // ... the states and the counts (n_terms entries each)
    // pfac_documents_rules (the sort's buffers, the ballots and the block prefixes are the term counts': both are used up
    // on the stream)
    uint64_t tc_table = 0;                // the table the slot's last term counts ran with (pfac_ctx::table_gen)
    DevBuf<unsigned> ru_cpre;             // per pair: the keys in front of it in its group of 4096 pairs, ...
    DevBuf<unsigned> ru_doc;              // ... and its document
    DevBuf<unsigned long long> ru_gsum;   // the keys per group of pairs, their prefix, the total E and the error word
    PassOut<unsigned long long> ru_row;   // row_ptr (n_docs + 1 entries), ...
    PassOut<unsigned> ru_out;             // ... and the fired rules (n_fired entries)
    // pfac_documents_near
    pfac_near_rule nr_host[PFAC_NEAR_MAX_RULES];  // the call's rules, copied from the caller's array (the upload reads these), ...
    DevBuf<pfac_near_rule> nr_rules;      // ... on the device, ...
    DevBuf<unsigned long long> nr_tab;    // ... per (rule, side) and block of 4096 records: the last A / B, then the block's carry-in
    PassOut<unsigned long long> nr_out;   // the masks (n_docs of them); scratch of a call that writes to the caller's buffer
    // pfac_documents_gather
    DevBuf<unsigned long long> ga_x;      // X per block of 64 ids
    PassOut<unsigned char> ga_out;        // the bytes, ...
    PassOut<unsigned long long> ga_off;   // ... and the output offsets (n_ids + 1 entries)
    // pfac_tokenize_leftmost_longest / pfac_tokenize_documents
    DevBuf<unsigned long long> tk_first;  // per tile: its first pick (n_tiles + 1 entries), ...
    DevBuf<unsigned long long> tk_bm;     // ... its 64 words of emitting positions, ...
    DevBuf<unsigned short> tk_wpre;       // ... the tokens in front of each word, ...
    DevBuf<unsigned> tk_tpre;             // ... and the tokens in front of the tile in its group of 64
    PassOut<int> tk_ids;                  // the token ids, ...
    PassOut<unsigned> tk_pos;             // ... their positions (PFAC_TOKENS_POSITIONS), ...
    PassOut<unsigned long long> tk_off;   // ... and the documents' token offsets (n_docs + 1 entries)
    // pfac_records_filter_roles / pfac_wordpiece_leftmost_longest / pfac_wordpiece_documents (first, bm, wpre, tpre and
    // the three outputs are the tokenizer's)
    bool rf_done = false;                 // the slot's last scan went through the role filter, ...
    uint64_t rf_gen = 0;                  // ... under this attachment (pfac_ctx::wp_gen)
    DevBuf<unsigned long long> wp_maps;   // per tile: W, U, ST, E0 (4 x 64 words), ...
    DevBuf<unsigned long long> wp_sum;    // ... its edge summary, ...
    DevBuf<unsigned long long> wp_unk;    // ... and its 64 words of [UNK] positions
    // pfac_unigram_records / pfac_unigram_documents (bm, wpre, tpre and the three outputs are the tokenizer's)
    DevBuf<unsigned long long> ug_maps;   // per tile: W, S, B (3 x 64 words)
    uint64_t ug_gen = 0;                  // the attachment the slot's token result was made under (pfac_ctx::ug_gen; 0: another pass)
    // pfac_bpe_records / pfac_bpe_documents (bm, wpre, tpre and the three outputs are the tokenizer's)
    DevBuf<unsigned long long> bpe_maps;  // per tile: V, P (2 x 64 words)
    uint64_t bpe_gen = 0;                 // the attachment the slot's token result was made under (pfac_ctx::bpe_gen; 0: another pass)
};

struct StageLayout {                      // per-wave LDS of one staging mode
    int nbuf = 2, pw_bytes = 0, waves_per_block = 0, lds_bytes = 0;
    unsigned stage_cap = 0;               // records per buffer (0: final states do not fit the packed word)
};

// Tuning and test knobs: the environment as ONE install reads it (read_knobs), once, before anything is built.
struct Knobs {
    bool force_l2 = false, no_d1 = false, no_fuse = false, no_d1pack = false, no_secf = false, no_nw4 = false, no_dense2 = false, verbose = false;
    int l2f = -1;                         // PFAC_L2F 0: filter off; 2: lookup form even where the SWAR / flag-only form applies; 3: flags only
    int nwb = 0, lag = 0;                 // PFAC_NWB: fewer waves per workgroup; PFAC_LAG 1 / 2: pin the emission lag (tests, A/B runs)
    int rec_bytes = 0, d2_logcap = 0;     // PFAC_REC_BYTES / _WIDE: a WIDER record form; PFAC_D2_LOGCAP: tiles with more records take the fallback pass
    int dense = -1;                       // PFAC_DENSE=0/1 pins the staging mode
    unsigned ticket_ways = 0, count_bins = 0, count_grid = 0, count_threads = 0;   // PFAC_TICKET_WAYS, PFAC_COUNT_BINS / _GRID / _THREADS (0: the defaults)
    unsigned terms_rows = 0;              // PFAC_TERMS_ROWS: workgroups of a sort pass of pfac_documents_term_counts (0: PFAC_TERMS_SORT_ROWS)
    unsigned spin_max = SPIN_MAX, fault = 0;                      // (they go into ScanArgs as they are)
    std::string trace_file;
};

// Everything ONE installed table fixes about the scans that run with it.  install_table builds it aside and moves it
// into the context whole, or not at all: no scan ever launches from a plan that an install has left half made.  What a
// kernel argument already says (the header's num_final, wbit, r_words = max_row, ht_size; the table views s0, r, T; the
// level-2 filter, the dense rows' numbers, the shared LDS carve, the root) is kept in `base` only.
struct TablePlan {
    DevBuf<unsigned char> tab;            // the repacked tables: base.s0, base.r, base.T and ...
    const int *d_idmap = nullptr;         // ... final state -> pattern id
    DevBuf<int> d1;                       // dense depth-1 rows + (after them) the 256-byte row index
    DevBuf<unsigned char> bm2;            // level-2 filter: 2-byte-prefix bitmap, 256 rows of 32 bytes, + the second-byte flags
    DevBuf<int4> T4_alloc;                // fused slots (variant 1, width >= 256), from slot min(0, min r) = -base.rn_bias
    int max_pat_len = 0, state_num = 0;   // header facts that no kernel argument carries
    ScanArgs base{};                      // every argument that does not change between uploads; a launch adds the rest
    int variant = 1;                      // 0: tables in LDS, 1: via L2
    bool fused = false;                   // ... as fused slots, one gather per step
    int root_mode = 0;                    // 1: the root has ONE edge, exact SWAR root test; 0: LDS flag tables
    StageLayout lay[2];                   // sparse staging: [0] two buffers (emission lags one round), [1] three (two rounds)
    StageLayout lay_d;                    // dense staging: one big buffer per wave (stage_cap 0: dense mode unavailable)
    bool lag2_ok = false;                 // the three-buffer layout is usable
    bool dense2 = false;                  // dense mode runs in its second form (dense2_tile): fused tables, packed dense rows, 4-byte records
    int grid_blocks = 0;
    const void *kernel[2] = {};           // [0] the exact kernel, [1] its twin that folds the input's case (pfac_ctx::fold chooses)
    const void *kernel_d[2] = {};         // the kernel dense mode launches (four walks per lane on fused L2 tables)
    const void *kernel3[2] = {};          // the three-staging-buffer twin of `kernel`
    Knobs knobs;
    const void *kernel_of(bool dense, bool lag2, unsigned fold) const { return dense ? kernel_d[fold] : (lag2 ? kernel3[fold] : kernel[fold]); }
    int max_lds() const { return std::max(lay_d.lds_bytes, std::max(lay[0].lds_bytes, lay[1].lds_bytes)); }
};

}  // namespace

struct pfac_ctx {
    int device = 0;
    int n_cu = 0;
    std::vector<Slot> slots;
    hipStream_t copy_stream = nullptr;    // every pfac_slot_h2d goes through this ONE stream, in call order: copies queued back to
                                          // back on one DMA queue run at the link's rate (55 GB/s), copies that alternate with
                                          // kernels on the slots' own streams leave gaps (45 GB/s measured); the slot's stream
                                          // waits for its copy through an event
    // table: what the installed one fixes, ...
    TablePlan plan;
    bool have_table = false;
    uint64_t table_gen = 0;               // installs begun so far: a scan's final states index the lengths of ITS table only
    // ... what the caller attaches to it (an upload drops all of it), ...
    DevBuf<short> flen;                   // pattern length of every final state (pfac_table_set_final_lengths)
    DevBuf<unsigned> rep_off;             // replacement of every final state (pfac_table_set_replacements): offsets[num_final + 1]
    DevBuf<unsigned char> rep;            // ... and the bytes, zero-padded to its capacity (a multiple of 16)
    DevBuf<unsigned> rep_split;           // where a state's replacement quotes the match (pfac_table_set_replacement_templates);
                                          // null while every state is plain: the replaces then run their plain kernels
    DevBuf<unsigned long long> gmask;     // group set of every final state (pfac_table_set_state_groups)
    DevBuf<int> sweight;                  // weight of every final state (pfac_table_set_state_weights)
    DevBuf<uint4> spans;                  // span of every final state (pfac_table_set_state_spans): pfac_state_span as one dwordx4
    DevBuf<int> tok;                      // token id of every final state (pfac_table_set_token_ids), PFAC_TOKEN_DROP = none, ...
    DevBuf<int> btok;                     // ... and of every byte value (256 entries; all DROP when the caller gave none)
    DevBuf<int2> wp_ids;                  // WordPiece (pfac_table_set_wordpiece): (first id, continuation id) of every final state, ...
    DevBuf<int> wp_btok;                  // ... the id of every byte value, ...
    int wp_unk = 0;                       // ... the id of a bad word, ...
    unsigned wp_max = 0;                  // ... the longest good word in bytes, ...
    WordSet wp_ws{};                      // ... and the word bytes
    uint64_t wp_gen = 0;                  // attachments made so far: a role filter remembers the one it ran under
    DevBuf<int4> ug_pieces;               // Unigram (pfac_table_set_unigram): (first id, cont id, first score, cont score) of every final state, ...
    DevBuf<int> ug_btok;                  // ... the id of every byte value, ...
    int ug_unk = 0, ug_bscore = 0;        // ... the id of a run of byte edges (or DROP: byte fallback), the score of a byte edge, ...
    unsigned ug_max = 0;                  // ... the longest word with piece edges, in bytes, ...
    WordSet ug_ws{};                      // ... and the word bytes
    uint64_t ug_gen = 0;                  // attachments made so far
    DevBuf<int4> bpe_pieces;              // BPE (pfac_table_set_bpe): (id, rank, split, 0) of every final state, ...
    DevBuf<int> bpe_btok;                 // ... the id of every byte value, ...
    int bpe_lead = -1;                    // ... the byte in front of a run that belongs to its word (or -1), ...
    unsigned bpe_max = 0;                 // ... the longest word that is merged, in bytes, ...
    WordSet bpe_ws{};                     // ... and the word bytes
    uint64_t bpe_gen = 0;                 // attachments made so far
    DevBuf<unsigned> ru_sptr;             // the rule table, state-major (pfac_table_set_rules): state_ptr[num_final + 1], ...
    DevBuf<unsigned> ru_ent;              // ... the entries rule << 1 | negated, the rules ascending inside a state, ...
    DevBuf<unsigned> ru_need;             // ... and need[n_rules]
    uint64_t ru_n = 0, ru_terms = 0;      // its rules (0: none) and its entries
    unsigned fold = PFAC_FOLD_NONE;       // case fold of the scans to come (pfac_table_set_case_fold)
    // ... and what adapts to the match density seen by the last scan (pfac_scan_finish)
    bool dense = false;                   // staging mode
    bool lag2 = false;                    // three-buffer layout in use
    bool run_dense() const { return dense && plan.lay_d.stage_cap; }       // ... of the next launch
    const StageLayout &layout(bool dense_mode) const { return dense_mode ? plan.lay_d : plan.lay[lag2 ? 1 : 0]; }
    bool event_timing = false;            // PFAC_EVENT_TIMING=1 (read when the context is created): the scan's dispatch carries a
                                          // start and a stop event, completion and pfac_scan_elapsed_ms come from them -- the
                                          // earlier form, kept to compare the two clocks and the two boundaries on one build
    double tick_ms = 1e-5;                // one tick of the kernel's clock (s_memrealtime) in ms: 1 / hipDeviceAttributeWallClockRate
    double clk_diff_ms = 0;               // PFAC_EVENT_TIMING: event time - the kernel's own, summed over the timed scans, ...
    uint64_t clk_n = 0;                   // ... and how many (printed when the context goes, under PFAC_VERBOSE)
    std::string err;
    std::mutex mu;
};

namespace {

int fail(pfac_ctx *ctx, int code, const std::string &msg) {
    g_err = msg;
    if (ctx) ctx->err = msg;
    return code;
}

// Every entry point works on its context's device and leaves the calling thread's current device as it found it
// (a caller that drives several GPUs from one thread -- torch does -- must not have it changed under its feet).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define USE_DEVICE(ctx)                                                                                    \
    DeviceGuard device_guard_((ctx)->device);                                                              \
    if (device_guard_.err != hipSuccess)                                                                   \
        return fail(ctx, PFAC_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(device_guard_.err))

int check_slot(pfac_ctx *ctx, int slot) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    if (slot < 0 || slot >= (int)ctx->slots.size()) return fail(ctx, PFAC_E_ARG, "bad slot index");
    return PFAC_OK;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// [first, first + n) within a result of `total` elements (subtracting: first + n may wrap)
bool in_window(uint64_t first, uint64_t n, uint64_t total) { return first <= total && n <= total - first; }

// One fetch of a slot-owned result: elements [first, first + n) of `o` to `host`, asynchronous on the slot's stream
// (whole-result fetches pass 0, o.n).  Checked in this order: `pass` has finished, else PFAC_E_STATE; `optional` and no
// host pointer: the half of a pair fetch that the caller does not want; the result is the slot's, else PFAC_E_STATE;
// the window lies in it and there is a host pointer where elements are asked for, else PFAC_E_ARG.
template <typename T>
int fetch(pfac_ctx *ctx, Slot &s, const PassOut<T> &o, const std::string &fn, const char *pass, void *host, uint64_t first,
          uint64_t n, bool optional = false) {
    if (!o.done) return fail(ctx, PFAC_E_STATE, fn + " without a finished " + pass);
    if (optional && !host) return PFAC_OK;
    if (!o.own) return fail(ctx, PFAC_E_STATE, fn + ": the last " + pass + " wrote into the caller's buffer");
    if (!in_window(first, n, o.n)) return fail(ctx, PFAC_E_ARG, fn + ": [first, first + n) exceeds the result of the last " + pass);
    if (!host && n) return fail(ctx, PFAC_E_ARG, fn + ": null host buffer");
    USE_DEVICE(ctx);
    if (n) HIP_TRY(ctx, hipMemcpyAsync(host, o.buf.p + first, n * sizeof(T), hipMemcpyDeviceToHost, s.stream));
    return PFAC_OK;
}

constexpr size_t CTL_REGION = (CTL_WORDS * 4 + 255) / 256 * 256;

int ensure_ctl(pfac_ctx *ctx, Slot &s) {
    if (s.ctl.p) return PFAC_OK;
    int rc = s.ctl.ensure(ctx, s.stream, 1, 2 * CTL_REGION / 4);
    if (rc) return rc;
    s.d_ctlbuf[0] = s.ctl.p;
    s.d_ctlbuf[1] = s.ctl.p + CTL_REGION / 4;
    s.clean[0] = s.clean[1] = false;
    s.flip = 0;
    return PFAC_OK;
}

// n_groups prefixes + the grand total behind them (callers that keep more words behind the total ask for more groups)
int ensure_gsum(pfac_ctx *ctx, Slot &s, unsigned n_groups) {
    return s.gsum.ensure(ctx, s.stream, (uint64_t)n_groups + 1, quarter_more(n_groups) + 1);
}

// a slot-owned array of n_docs + 1 entries (offsets, doc_first)
int ensure_docs(pfac_ctx *ctx, Slot &s, DevBuf<unsigned long long> &b, uint64_t n_docs) {
    return b.ensure(ctx, s.stream, n_docs + 1, docs_cap(n_docs));
}

// f(std::integral_constant<int, BYTES>()) for a record width of 2, 4 or 8 bytes: how a pass picks the kernel of the
// last scan's record form, as in  by_width(rb, [](auto w) { return pfac_expand_kernel<w()>; })
template <typename F>
auto by_width(int rec_bytes, F f) {
    return rec_bytes == 2 ? f(std::integral_constant<int, 2>()) : (rec_bytes == 4 ? f(std::integral_constant<int, 4>()) : f(std::integral_constant<int, 8>()));
}

uint64_t host_u64(const Slot &s, int word) { return ((uint64_t)s.h_ctl[word + 1] << 32) | s.h_ctl[word]; }

// The result words of a pass, from behind its group prefixes into h_ctl (read them with host_u64): the launch-error
// check of the kernels that made them, the copy, and the ONE synchronise a pass spends on learning its total.
int pass_words(pfac_ctx *ctx, Slot &s, const unsigned long long *dev, int n_words, int first_word = H_PASS) {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + first_word, dev, (size_t)n_words * 8, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    return PFAC_OK;
}

// The sort of pfac_documents_term_counts and pfac_documents_rules: n 8-byte keys in the first half of s.tc_keys (2 n
// entries), a stable LSD radix sort over `passes` digits of TOP_BITS bits.  A workgroup takes `chunks` chunks of TC_BLOCK
// keys, so that a pass has PFAC_TERMS_SORT_ROWS workgroups at most (the PFAC_TERMS_ROWS knob); n <= TC_BLOCK keys are
// sorted by one workgroup.  tc_sort_reserve grows the digit counts (before the first launch that writes the keys: growing
// waits for the stream); tc_sort queues the passes and returns the half that holds the sorted keys.
struct TcSortShape {
    unsigned chunks, n_blocks;
    bool one;
};
TcSortShape tc_sort_shape(const pfac_ctx *ctx, uint64_t n) {
    const uint64_t n_chunks = (n + TC_BLOCK - 1) / TC_BLOCK;
    const uint64_t rows = ctx->plan.knobs.terms_rows ? ctx->plan.knobs.terms_rows : PFAC_TERMS_SORT_ROWS;
    const unsigned chunks = (unsigned)std::max<uint64_t>(1, (n_chunks + rows - 1) / rows);
    return TcSortShape{chunks, (unsigned)((n_chunks + chunks - 1) / chunks), n <= (uint64_t)TC_BLOCK};
}
int tc_sort_reserve(pfac_ctx *ctx, Slot &s, uint64_t n, int passes) {
    const TcSortShape sh = tc_sort_shape(ctx, n);
    if (sh.one || !passes) return PFAC_OK;
    return s.tc_bh.ensure(ctx, s.stream, (uint64_t)TOP_BINS * (sh.n_blocks + 1), (uint64_t)TOP_BINS * (quarter_more(sh.n_blocks) + 1));
}
const unsigned long long *tc_sort(pfac_ctx *ctx, Slot &s, uint64_t n, int passes) {
    const TcSortShape sh = tc_sort_shape(ctx, n);
    const unsigned chunks = sh.chunks, n_blocks = sh.n_blocks;
    unsigned long long *a = s.tc_keys.p, *b = s.tc_keys.p + n;
    if (sh.one && passes) {
        hipLaunchKernelGGL(pfac_tc_sort_one_kernel, dim3(1), dim3(TS_WAVES * WAVE), 0, s.stream, a, (unsigned long long)n, passes);
    } else {
        unsigned *tot = s.tc_bh.p + (uint64_t)TOP_BINS * n_blocks;
        for (int pass = 0; pass < passes; pass++) {
            hipLaunchKernelGGL(pfac_tc_sort_hist_kernel, dim3(n_blocks), dim3(TS_WAVES * WAVE), 0, s.stream, (const unsigned long long *)a,
                               (unsigned long long)n, pass * TOP_BITS, chunks, n_blocks, s.tc_bh.p);
            hipLaunchKernelGGL(pfac_tc_sort_rows_kernel, dim3(TOP_BINS), dim3(TS_WAVES * WAVE), 0, s.stream, s.tc_bh.p, n_blocks, tot);
            hipLaunchKernelGGL(pfac_tc_sort_scatter_kernel, dim3(n_blocks), dim3(TS_WAVES * WAVE), 0, s.stream, (const unsigned long long *)a,
                               (unsigned long long)n, pass * TOP_BITS, chunks, n_blocks, (const unsigned *)s.tc_bh.p, (const unsigned *)tot, b);
            std::swap(a, b);
        }
    }
    return a;
}

// What a pass needs of the slot's last scan, tested in this order (the first failure is the one reported).
enum : unsigned {
    SCAN_FINISHED = 1,                    // there is one, and pfac_scan_finish has returned
    SCAN_LENGTHS = 2,                     // the uploaded table has its final-state lengths
    SCAN_TABLE = 4,                       // it ran with the table that is installed now, ...
    SCAN_IDMAP = 8,                       // ... (the same, for a pass that maps its states through that table's idmap)
    SCAN_FITS = 16,                       // its records fitted the heap
};
int last_scan_usable(pfac_ctx *ctx, const Slot &s, const std::string &fn, unsigned what) {
    if ((what & SCAN_FINISHED) && (!s.scanned || s.pending)) return fail(ctx, PFAC_E_STATE, fn + " needs a finished scan");
    if ((what & SCAN_LENGTHS) && (!ctx->have_table || !ctx->flen.p))
        return fail(ctx, PFAC_E_STATE, fn + ": no final-state lengths for the uploaded table (pfac_table_set_final_lengths)");
    if ((what & (SCAN_TABLE | SCAN_IDMAP)) && s.last_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's last scan ran with an earlier table" +
                                           ((what & SCAN_IDMAP) ? " (its states index that table's idmap)" : ""));
    if ((what & SCAN_FITS) && s.last_used > s.last_cap)
        return fail(ctx, PFAC_E_OVERFLOW, "the slot's last scan overflowed its record heap: scan again with a larger one");
    return PFAC_OK;
}

// The documents argument of a pass: NULL means the slot's offsets (pfac_slot_doc_offsets), and then n_docs must be
// theirs; `others` are the bits of the pass's other document-sized device pointers, which share the alignment rule.
int resolve_docs(pfac_ctx *ctx, const Slot &s, const std::string &fn, const uint64_t *d_doc_offsets, uint64_t n_docs,
                 uintptr_t others, const unsigned long long **off) {
    *off = reinterpret_cast<const unsigned long long *>(d_doc_offsets);
    if (!*off) {
        if (!s.doc.done) return fail(ctx, PFAC_E_STATE, fn + ": no document offsets for the slot (pfac_slot_doc_offsets)");
        if (n_docs + 1 != s.doc.n) return fail(ctx, PFAC_E_ARG, fn + ": n_docs differs from the slot's document offsets");
        *off = s.doc.buf.p;
    }
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if (n_docs == 0 && s.last_owned != 0) return fail(ctx, PFAC_E_ARG, fn + ": no documents, but the scan owns bytes");
    if (((uintptr_t)*off | others) & 7) return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    return PFAC_OK;
}

int bad_doc_offsets(pfac_ctx *ctx, const Slot &s, const std::string &fn) {     // (the device found them so)
    return fail(ctx, PFAC_E_ARG, fn + ": document offsets must start at 0, not decrease, and end at the scan's n_owned (" +
                                     std::to_string(s.last_owned) + ")");
}

// Tuning and test knobs (PFAC_FORCE_L2, PFAC_NWB, PFAC_FAULT, ...) are honoured ONLY in a process that opts in with
// PFAC_ENABLE_KNOBS=1 (the tests and the tools do): a production process cannot have its scans altered -- or a fault injected
// -- by a stray environment variable.
const char *knob(const char *name) {
    static const bool enabled = [] { const char *v = getenv("PFAC_ENABLE_KNOBS"); return v && *v && *v != '0'; }();
    return enabled ? getenv(name) : nullptr;
}
int env_int(const char *name, int dflt) {
    const char *v = knob(name);
    return v && *v ? atoi(v) : dflt;
}

// Waits for the slot's last scan -- for IT, not for the stream: another slot may share the stream (launch pipelining), and
// its scan, enqueued behind this one, keeps the GPU busy while the host reads this result.  The kernel's last workgroup
// stores H_DONE behind the other result words; the host polls that word.  Nothing is queued on the stream meanwhile (no
// query, no event): a signalled packet between two scans is what the dispatch no longer pays for.  The poll is bounded
// by Slot::spin_ms, a generous multiple of the scan's time; past it the stream itself is waited for, and a stream that
// has gone idle with the word still unset is an error, as is one that failed.
int wait_scan(pfac_ctx *ctx, Slot &s) {
    if (ctx->event_timing) { HIP_TRY(ctx, hipEventSynchronize(s.ev1)); return PFAC_OK; }
    const volatile unsigned *done = s.h_ctl + H_DONE;
    auto is_done = [&] { return __atomic_load_n(done, __ATOMIC_ACQUIRE) != 0; };
    if (is_done()) return PFAC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        for (int i = 0; i < 64; i++) {
            if (is_done()) return PFAC_OK;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > s.spin_ms) break;
    }
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    if (!is_done()) return fail(ctx, PFAC_E_INTERNAL, "the scan's stream is idle, but the scan has not reported its completion");
    return PFAC_OK;
}

// The scan kernel of a table placement (0: tables via L2, 1: tables in LDS, 2: fused L2 tables, 3: fused L2 tables
// with four walks per lane -- dense mode, two staging buffers only), hash width, root test, NB staging buffers and case
// fold (every kernel has a twin that folds its tile on the way into LDS).
template <int NB, bool TLDS, bool FUSED, int NW, bool FOLD>
const void *scan_kernel_of(bool w8, int root) {
    const void *const k[2][2] = {
        {(const void *)pfac_scan_kernel<TLDS, false, 0, FUSED, NW, NB, FOLD>, (const void *)pfac_scan_kernel<TLDS, false, 1, FUSED, NW, NB, FOLD>},
        {(const void *)pfac_scan_kernel<TLDS, true, 0, FUSED, NW, NB, FOLD>, (const void *)pfac_scan_kernel<TLDS, true, 1, FUSED, NW, NB, FOLD>}};
    return k[w8 ? 1 : 0][root];
}
template <int NB, bool FOLD>
const void *scan_kernel_fold(int placement, bool w8, int root) {
    // (three walks per lane for the sparse fused kernels -- one round per tile of the 75 840-pattern set on random bytes
    // instead of 1.45 -- measured 3 % slower than two: 112 VGPRs and the longer round cost more than the second round)
    constexpr int FNW = PFAC_SPARSE_FUSED_NW;   // walks per lane of the sparse-mode kernels on fused L2 tables
    switch (placement) {
    case 0: return scan_kernel_of<NB, false, false, 2, FOLD>(w8, root);
    case 1: return scan_kernel_of<NB, true, false, 1, FOLD>(w8, root);
    case 2: return scan_kernel_of<NB, false, true, FNW, FOLD>(w8, root);
    default: return scan_kernel_of<2, false, true, 4, FOLD>(w8, root);
    }
}
template <int NB>
const void *scan_kernel(int placement, bool w8, int root, unsigned fold) {
    return fold ? scan_kernel_fold<NB, true>(placement, w8, root) : scan_kernel_fold<NB, false>(placement, w8, root);
}

// layout of TablePlan::d1: rows (d1_rows x 256 int32) | 256-byte row index | the depth-1 states | (packed rows) {r[], child
// mask} of the depth-2 states (8-byte aligned) | counter | column map | column bytes
size_t d1_off_r2(int d1_rows) { return align_up((size_t)d1_rows * 1024 + 256 + (size_t)d1_rows * 4, 8); }
size_t d1_off_col(int d1_rows) { return d1_off_r2(d1_rows) + (size_t)D1_N2_MAX * 8 + 16; }

// ---- install, step 1: every knob, read once per table install
Knobs read_knobs() {
    Knobs k;
    auto is_set = [](const char *name) { return knob(name) != nullptr; };
    k.force_l2 = is_set("PFAC_FORCE_L2");                  // tuning knob: tables via L2 even if they fit LDS
    k.no_d1 = is_set("PFAC_NO_D1"); k.no_d1pack = is_set("PFAC_NO_D1PACK"); k.no_fuse = is_set("PFAC_NO_FUSE");
    k.no_secf = is_set("PFAC_NO_SECF"); k.no_nw4 = is_set("PFAC_NO_NW4"); k.no_dense2 = is_set("PFAC_NO_DENSE2");
    k.verbose = is_set("PFAC_VERBOSE");
    k.l2f = env_int("PFAC_L2F", -1);
    k.nwb = env_int("PFAC_NWB", 0);
    k.lag = env_int("PFAC_LAG", 0);
    k.rec_bytes = env_int("PFAC_REC_BYTES", is_set("PFAC_WIDE") ? 8 : 0);
    k.d2_logcap = env_int("PFAC_D2_LOGCAP", 0);
    k.dense = is_set("PFAC_DENSE") ? atoi(knob("PFAC_DENSE")) : -1;
    k.spin_max = std::max(64u, (unsigned)env_int("PFAC_SPIN_MAX", (int)SPIN_MAX));
    k.fault = (unsigned)env_int("PFAC_FAULT", 0);
    k.ticket_ways = (unsigned)env_int("PFAC_TICKET_WAYS", 0);
    k.trace_file = is_set("PFAC_TRACE") ? knob("PFAC_TRACE") : "";
    // the state histogram: a smaller LDS table (the cache regime and its collisions at small automata), a fixed grid
    const int cbins = env_int("PFAC_COUNT_BINS", 0), cgrid = env_int("PFAC_COUNT_GRID", 0), cthreads = env_int("PFAC_COUNT_THREADS", 0);
    k.count_bins = cbins >= 1 && (unsigned)cbins <= COUNT_BINS_MAX ? (unsigned)cbins : 0u;
    k.count_grid = cgrid >= 1 ? (unsigned)std::min(cgrid, 65536) : 0u;
    k.count_threads = cthreads == 256 || cthreads == 512 || cthreads == 1024 ? (unsigned)cthreads : 0u;
    // the term counts' sort: another limit on the workgroups (histogram rows) of a pass
    const int trows = env_int("PFAC_TERMS_ROWS", 0);
    k.terms_rows = trows >= 1 ? (unsigned)std::min(trows, 1 << 20) : 0u;
    return k;
}

// The root's edges, as the repacked tables have them.
struct RootFan {
    int32_t s0[256];
    int fan = 0, last = 0;                // edges, and the byte of the last one (fan == 1: of the only one)
    int state[256];                       // the depth-1 states, by edge ...
    unsigned char idx[256];               // ... and root byte -> edge (its dense row)
};

// ---- the tables themselves: the image repacked into P.tab (on `stream`), its header facts and views, the root's edges.
// d_blob: device-resident blob image; hdr: its first 16 words on the host, already checked
int plan_tables(pfac_ctx *ctx, TablePlan &P, const int *d_blob, const int32_t *hdr, hipStream_t stream, RootFan &root) {
    const int width = hdr[2], wbit = hdr[3], num_final = hdr[5], state_num = hdr[6], max_row = hdr[8], ht_size = hdr[9];
    const size_t off_r = 256 * 4, off_T = align_up(off_r + (size_t)max_row * 4, 16), off_id = off_T + (size_t)ht_size * 8;
    const size_t total = align_up(off_id + (size_t)num_final * 4, 16) + 16;
    if (int rc = P.tab.ensure(ctx, nullptr, total, total)) return rc;
    unsigned char *base = P.tab.p;
    int *d_s0 = reinterpret_cast<int *>(base), *d_r = reinterpret_cast<int *>(base + off_r);
    int2 *d_T = reinterpret_cast<int2 *>(base + off_T);
    int *d_idmap = reinterpret_cast<int *>(base + off_id), *d_bad = reinterpret_cast<int *>(base + total - 16);
    HIP_TRY(ctx, hipMemsetAsync(d_bad, 0, 4, stream));
    hipLaunchKernelGGL(pfac_repack_kernel, dim3(256), dim3(256), 0, stream, d_blob, d_s0, d_r, d_T, d_idmap, max_row, ht_size,
                       num_final, state_num, width, d_bad);
    HIP_TRY(ctx, hipGetLastError());
    int bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (bad) return fail(ctx, PFAC_E_ARG, "table image: a displacement or a state points outside the tables");
    ScanArgs &B = P.base;
    B.s0 = d_s0; B.r = d_r; B.T = d_T; P.d_idmap = d_idmap;
    B.r_words = max_row; B.t_entries = B.ht_size = ht_size; B.wbit = wbit; B.num_final = num_final; P.state_num = state_num; P.max_pat_len = hdr[7];
    HIP_TRY(ctx, hipMemcpy(root.s0, d_s0, sizeof root.s0, hipMemcpyDeviceToHost));
    for (int i = 0; i < 256; i++) {
        root.idx[i] = 0;
        if (root.s0[i] >= 0) { root.state[root.fan] = root.s0[i]; root.idx[i] = (unsigned char)(root.fan < 255 ? root.fan : 255); root.fan++; root.last = i; }
    }
    return PFAC_OK;
}

// ---- install, step 2: dense rows for the depth-1 states (children of the root), when there are few enough of them.
// Rows are built in device memory in full, 256 columns; LDS takes the columns that have an edge in some row.  On fused
// tables with few enough depth-2 states the rows are packed: an entry carries the index of its state's {r[], child mask}.
int plan_dense_rows(pfac_ctx *ctx, TablePlan &P, const RootFan &root) {
    ScanArgs &B = P.base;
    const int n_rows = (root.fan >= 1 && root.fan <= 255 && !P.knobs.no_d1) ? root.fan : 0;
    if (!n_rows) return PFAC_OK;
    const size_t off_r2 = d1_off_r2(n_rows), off_col = d1_off_col(n_rows);
    if (int rc = P.d1.ensure(ctx, nullptr, (off_col + 512) / 4, (off_col + 512) / 4)) return rc;
    unsigned char *b = reinterpret_cast<unsigned char *>(P.d1.p);
    int *d_state = reinterpret_cast<int *>(b + (size_t)n_rows * 1024 + 256);
    HIP_TRY(ctx, hipMemcpy(b + (size_t)n_rows * 1024, root.idx, 256, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(d_state, root.state, (size_t)n_rows * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pfac_build_d1_kernel, dim3(n_rows), dim3(256), 0, 0, d_state, B.r, B.T, B.wbit, B.ht_size, P.d1.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    // which bytes are the second byte of some pattern: the LDS rows keep those columns only (host copy of the
    // rows: at most 255 KiB); too many rows x columns for LDS: no dense level
    std::vector<int> rows((size_t)n_rows * 256);
    HIP_TRY(ctx, hipMemcpy(rows.data(), P.d1.p, rows.size() * 4, hipMemcpyDeviceToHost));
    unsigned char colmap[256], colbyte[256];
    int ncols = 0;
    for (int c = 0; c < 256; c++) {
        bool used = false;
        for (int f = 0; f < n_rows && !used; f++) used = rows[(size_t)f * 256 + c] >= 0;
        if (used) colbyte[ncols++] = (unsigned char)c;
    }
    const int stride = ncols < 256 ? ncols + 1 : 256;      // one more column, "no edge", unless every byte has its own
    for (int c = 0; c < 256; c++) colmap[c] = (unsigned char)(ncols & 255);
    for (int k = 0; k < ncols; k++) colmap[colbyte[k]] = (unsigned char)k;
    if ((size_t)n_rows * stride * 4 > (size_t)D1_LDS_MAX) { P.d1.reset(); return PFAC_OK; }
    HIP_TRY(ctx, hipMemcpy(b + off_col, colmap, 256, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(b + off_col + 256, colbyte, 256, hipMemcpyHostToDevice));
    B.d1 = P.d1.p; B.d1idx = b + (size_t)n_rows * 1024; B.d1_colmap = b + off_col; B.d1_colbyte = b + off_col + 256;
    B.d1_rows = n_rows; B.d1_stride = stride; B.d1_ncols = ncols;
    B.d1_lds_bytes = (int)align_up((size_t)(n_rows + 1) * stride * 4, 16);   // (+ one row without edges)
    if (!P.fused || P.state_num > (1 << D1_STATE_BITS) || P.knobs.no_d1pack) return PFAC_OK;
    int n2 = 0;                                             // how many depth-2 states are there?
    for (int v : rows) n2 += v >= 0;
    if (n2 < 1 || n2 > D1_N2_MAX) return PFAC_OK;
    int2 *r2 = reinterpret_cast<int2 *>(b + off_r2);
    int *counter = reinterpret_cast<int *>(r2 + D1_N2_MAX);
    HIP_TRY(ctx, hipMemset(counter, 0, 4));
    hipLaunchKernelGGL(pfac_pack_d1_kernel, dim3((unsigned)n_rows), dim3(256), 0, 0, P.d1.p, n_rows * 256, B.r, B.T, B.wbit,
                       B.ht_size, B.r_words, r2, counter);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    B.d1r2 = r2; B.d1_n2 = n2;
    return PFAC_OK;
}

// ---- install, step 3: the level-2 filter.  The 2-byte-prefix bitmap is built on the device from the uploaded tables; a
// single-edge root with at most two grandchildren gets the bit-parallel form (their bytes), everything else the lookup form
int plan_l2_filter(pfac_ctx *ctx, TablePlan &P, const RootFan &root) {
    ScanArgs &B = P.base;
    if (int rc = P.bm2.ensure(ctx, nullptr, 256 * 32 + 256, 256 * 32 + 256)) return rc;   // bitmap + the second-byte flags
    hipLaunchKernelGGL(pfac_build_bm2_kernel, dim3(256), dim3(256), 0, 0, B.s0, B.r, B.T, B.wbit, B.ht_size,
                       reinterpret_cast<unsigned long long *>(P.bm2.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    B.bm2 = P.bm2.p; B.sec2 = P.bm2.p + 256 * 32;
    B.l2f_mode = 2; B.bm2_rows = 256;
    std::vector<unsigned char> bm2_host(256 * 32 + 256);
    HIP_TRY(ctx, hipMemcpy(bm2_host.data(), P.bm2.p, 256 * 32, hipMemcpyDeviceToHost));
    for (int c = 0; c < 256; c++) {                         // column OR: can byte c be a pattern's second byte?
        unsigned char any = 0;
        for (int b0 = 0; b0 < 256; b0++) any |= (unsigned char)(bm2_host[(size_t)b0 * 32 + (c >> 3)] >> (c & 7) & 1);
        bm2_host[256 * 32 + c] = any;
    }
    HIP_TRY(ctx, hipMemcpy(P.bm2.p + 256 * 32, bm2_host.data() + 256 * 32, 256, hipMemcpyHostToDevice));
    bool any_fin1 = false;                                  // a 1-byte pattern: its survivors are kept whatever follows
    for (int i = 0; i < 256; i++) any_fin1 = any_fin1 || (root.s0[i] >= 0 && root.s0[i] < B.num_final);
    B.sec_filter = (root.fan != 1 && !any_fin1 && !P.knobs.no_secf) ? 1 : 0;
    if (root.fan == 1) {
        const unsigned char *row = bm2_host.data() + (size_t)root.last * 32;
        int nch = 0, ch[2] = {0, 0};
        for (int c = 0; c < 256; c++)
            if (row[c >> 3] >> (c & 7) & 1) { if (nch < 2) ch[nch] = c; nch++; }
        B.bm2_rows = 1;
        if (nch <= 2) {
            B.l2f_mode = 1; B.n_child = nch;
            B.child0 = (unsigned)ch[0] * 0x01010101u;
            B.child1 = (unsigned)ch[nch > 1 ? 1 : 0] * 0x01010101u;
        }
    }
    // multi-edge root without 1-byte patterns: when most (first byte, second byte) combinations of the flagged bytes
    // ARE 2-byte prefixes, the bitmap lookup would drop few of the survivors the second-byte flags let through -- they
    // all go to the walk instead (mode 3), whose dense depth-1 row is the same lookup done 64 lanes wide
    if (root.fan != 1 && B.sec_filter) {
        long pairs = 0, nsec = 0;
        for (int i = 0; i < 256 * 32; i++) pairs += __builtin_popcount(bm2_host[(size_t)i]);
        for (int c = 0; c < 256; c++) nsec += bm2_host[256 * 32 + c];
        if (nsec > 0 && pairs * 100 >= (long)root.fan * nsec * PFAC_PAIR_DENSITY_PCT) B.l2f_mode = 3;
    }
    if (P.knobs.l2f == 0) B.l2f_mode = 0;
    else if (P.knobs.l2f == 2) B.l2f_mode = 2;
    else if (P.knobs.l2f == 3 && root.fan != 1 && B.sec_filter) B.l2f_mode = 3;
    return PFAC_OK;
}

// table bytes if staged in LDS: r (16-B rounded) + T
size_t lds_table_bytes(const ScanArgs &B) { return align_up((size_t)B.r_words * 4, 16) + (size_t)B.ht_size * 8; }
// one workgroup per CU: ask for more than half of the LDS so two never share a CU while another idles
int lds_of_one_block_per_cu(int lds_bytes) { return lds_bytes < LDS_TOTAL / 2 + 256 ? LDS_TOTAL / 2 + 256 : lds_bytes; }

// ---- install, step 4: the LDS carve -- plain arithmetic on what the steps before have put into the plan: no HIP call,
// no environment.  First the region every wave of a workgroup shares (its offsets go to the kernel: shared_bytes, sh_t0,
// sh_bm2), then one region per compute wave in each of the three staging modes.  False: not even one compute wave fits.
bool plan_lds(TablePlan &P) {
    ScanArgs &B = P.base;
    const Knobs &K = P.knobs;
    B.shared_bytes = SH_D1 + B.d1_lds_bytes + (P.variant == 0 ? (int)align_up(lds_table_bytes(B), 16) : (int)align_up((size_t)(B.d1_n2 ? B.d1_n2 + 1 : 0) * 8, 16));
    if (P.fused && B.d1_rows == 0) B.shared_bytes += 1024;   // r[] of the depth-1 states by root byte
    if (B.d1_n2 > 0) { B.sh_t0 = B.shared_bytes; B.shared_bytes += 1024; }   // dense mode, second form: its root table
    B.sh_bm2 = B.shared_bytes;
    if (B.l2f_mode == 2) B.shared_bytes += B.bm2_rows * 32;
    // The two-buffer layout fixes the number of waves; LDS that no further wave fits into goes to the staging buffers
    // (up to 1024 records per 4 KiB tile before it has to be walked a second time).  The three-buffer layout (emission
    // at the top of the round, see NBUF_MAX) is used when it keeps that many waves with room for >= CAPW3_MIN records.
    for (int nb = 2; nb <= NBUF_MAX; nb++) {
        StageLayout &L = P.lay[nb - 2];
        L.nbuf = nb;
        L.pw_bytes = (int)align_up((size_t)PW_FIXED_1BUF + (size_t)nb * CAPW * 4 + B.halo, 16);
        int nwb = (LDS_TOTAL - B.shared_bytes) / L.pw_bytes + 1;        // compute waves + the coordinator (no LDS region)
        if (nb == 3) {                                                  // as many waves as with two buffers, smaller buffers if need be
            nwb = P.lay[0].waves_per_block;
            L.pw_bytes = (int)align_up((size_t)PW_FIXED_1BUF + B.halo, 16);
        }
        if (nwb > MAX_WAVES_PER_BLOCK) nwb = MAX_WAVES_PER_BLOCK;
        if (K.nwb > 0 && K.nwb < nwb) nwb = K.nwb;
        if (nwb < 2) return false;
        L.waves_per_block = nwb;
        const int base_cap = nb == 3 ? 0 : CAPW;
        const int spare = (LDS_TOTAL - B.shared_bytes) / (nwb - 1) - L.pw_bytes;            // bytes per compute wave
        const int extra = spare > 0 ? (spare / (nb * 4)) & ~15 : 0;                         // records per staging buffer
        unsigned cap = (unsigned)(base_cap + ((K.nwb && nb == 2) ? 0 : extra));
        if (cap > 1024u) cap = 1024u;
        L.pw_bytes += (int)(cap - base_cap) * nb * 4;
        L.stage_cap = cap;
        L.lds_bytes = lds_of_one_block_per_cu(B.shared_bytes + (nwb - 1) * L.pw_bytes);
    }
    P.lag2_ok = P.lay[1].stage_cap >= (unsigned)CAPW3_MIN && K.lag != 1;
    if (B.rec_bytes == 8) {                                 // nothing is staged: every tile is written as it is walked
        P.lay[0].stage_cap = P.lay[1].stage_cap = 0u;
        P.lag2_ok = false;
    }
    // dense-mode layout; on fused L2 tables it runs four walks per lane, which needs <= MAX_WAVES_NW4 waves per workgroup
    StageLayout &D = P.lay_d;
    D.nbuf = 1;
    D.pw_bytes = (int)align_up((size_t)(P.dense2 ? PW_FIXED_DENSE2 : PW_FIXED_DENSE) + B.halo, 16);
    int nwd = (LDS_TOTAL - B.shared_bytes) / D.pw_bytes + 1;
    if (nwd > MAX_WAVES_PER_BLOCK) nwd = MAX_WAVES_PER_BLOCK;
    D.stage_cap = (nwd >= 4 && P.lay[0].stage_cap) ? (unsigned)CAPW_DENSE : 0u;   // 0: dense mode unavailable
    if (P.fused && !K.no_nw4 && !P.dense2 && nwd > MAX_WAVES_NW4) nwd = MAX_WAVES_NW4;
    D.waves_per_block = nwd;
    D.lds_bytes = lds_of_one_block_per_cu(B.shared_bytes + (nwd - 1) * D.pw_bytes);
    return true;
}

// ---- install, step 5: tables via L2 and PHF width >= 256: fused slots, one gather per step
int plan_fused_tables(pfac_ctx *ctx, TablePlan &P) {
    if (!P.fused) return PFAC_OK;
    ScanArgs &B = P.base;
    std::vector<int> r_host((size_t)B.r_words);
    HIP_TRY(ctx, hipMemcpy(r_host.data(), B.r, r_host.size() * 4, hipMemcpyDeviceToHost));
    long long lo = 0, hi = B.ht_size;
    for (int v : r_host) { lo = std::min<long long>(lo, v); hi = std::max(hi, (long long)v + (1 << B.wbit)); }
    if (hi - lo >= (1ll << 28)) return fail(ctx, PFAC_E_ARG, "table image: more than 2^28 hash slots");
    if (int rc = P.T4_alloc.ensure(ctx, nullptr, (uint64_t)(hi - lo), (uint64_t)(hi - lo))) return rc;
    B.T4 = P.T4_alloc.p;
    B.rn_bias = (int)-lo;
    hipLaunchKernelGGL(pfac_fuse_kernel, dim3(256), dim3(256), 0, 0, B.T, B.r, B.wbit, B.ht_size, B.r_words, P.T4_alloc.p - lo,
                       (int)lo, (int)hi);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    return PFAC_OK;
}

// ---- install, step 6: the kernels of this placement, hash width and root test, each allowed the largest LDS carve
int plan_kernels(pfac_ctx *ctx, TablePlan &P) {
    const bool w8 = P.base.wbit == 8;
    const int placement = P.variant == 0 ? 1 : (P.fused ? 2 : 0);
    const bool nw4 = P.fused && !P.knobs.no_nw4;           // dense mode on fused L2 tables: four walks per lane
    for (unsigned f = 0; f < 2; f++) {         // [1]: the twins that fold (pfac_table_set_case_fold chooses per launch)
        P.kernel[f] = scan_kernel<2>(placement, w8, P.root_mode, f);
        P.kernel_d[f] = nw4 ? scan_kernel<2>(3, w8, P.root_mode, f) : P.kernel[f];
        P.kernel3[f] = scan_kernel<3>(placement, w8, P.root_mode, f);
        for (const void *k : {P.kernel3[f], P.kernel_d[f], P.kernel[f]})
            HIP_TRY(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, P.max_lds()));
    }
    return PFAC_OK;
}

// The plan of one table image, every step in turn; any refusal leaves P to its caller, who drops it.
int build_plan(pfac_ctx *ctx, TablePlan &P, const int *d_blob, const int32_t *hdr, hipStream_t stream) {
    P.knobs = read_knobs();
    RootFan root;
    int rc = plan_tables(ctx, P, d_blob, hdr, stream, root);
    if (rc) return rc;
    ScanArgs &B = P.base;
    P.variant = lds_table_bytes(B) <= (size_t)LDS_TABLE_MAX && !P.knobs.force_l2 ? 0 : 1;
    P.fused = P.variant == 1 && B.wbit >= 8 && !P.knobs.no_fuse;
    B.halo = ((P.max_pat_len > 1 ? P.max_pat_len - 1 : 0) + 15) & ~15;
    // root fan-out 1 -> exact SWAR root test (ROOT = 1), else LDS flag tables (ROOT = 0)
    P.root_mode = root.fan == 1 ? 1 : 0;
    B.root_byte = (unsigned)root.last * 0x01010101u;
    B.root_state = root.s0[root.last];
    // records are as wide as the automaton needs: 12 position bits + the final state
    B.rec_bytes = B.num_final <= 16 ? 2 : (B.num_final <= (1 << PACK_STATE_BITS) ? 4 : 8);
    if ((P.knobs.rec_bytes == 4 || P.knobs.rec_bytes == 8) && (unsigned)P.knobs.rec_bytes > B.rec_bytes) B.rec_bytes = (unsigned)P.knobs.rec_bytes;
    B.spin_max = P.knobs.spin_max; B.fault = P.knobs.fault;
    P.grid_blocks = ctx->n_cu;
    if ((rc = plan_dense_rows(ctx, P, root))) return rc;
    if ((rc = plan_l2_filter(ctx, P, root))) return rc;
    P.dense2 = P.fused && !P.knobs.no_nw4 && !P.knobs.no_dense2 && B.d1_rows > 0 && B.d1_n2 > 0 && B.num_final <= 65535 && B.rec_bytes == 4;
    B.d2log_cap = P.knobs.d2_logcap >= 16 && (unsigned)P.knobs.d2_logcap < D2_LOG_CAP ? (unsigned)P.knobs.d2_logcap : D2_LOG_CAP;
    if (!plan_lds(P)) return fail(ctx, PFAC_E_INTERNAL, "LDS budget cannot hold one compute wave");
    B.sparse_cap = P.lay[0].stage_cap;     // tiles with more matches than these count towards the mode adaptation
    B.small_cap = P.lay[P.lag2_ok ? 1 : 0].stage_cap;
    if ((rc = plan_fused_tables(ctx, P))) return rc;
    if ((rc = plan_kernels(ctx, P))) return rc;
    if (P.knobs.verbose)
        fprintf(stderr, "pfac: variant %d fused %d shared LDS %d B; sparse: %d waves x %d B; dense%s: %d waves x %d B; dense rows %d x %d, %d depth-2 states, level-2 filter mode %d\n",
                P.variant, (int)P.fused, B.shared_bytes, P.lay[0].waves_per_block, P.lay[0].pw_bytes, P.dense2 ? " (second form)" : "",
                P.lay_d.waves_per_block, P.lay_d.pw_bytes, B.d1_rows, B.d1_stride, B.d1_n2, B.l2f_mode);
    return PFAC_OK;
}

// An upload.  A refused header leaves the installed table as it was.  Past the header checks the install is all or
// nothing: the old plan and what the caller attached to it are dropped first (so the old tables are gone before the new
// ones are allocated) and every earlier scan becomes one "made with an earlier table"; the new plan is built aside and
// moved into the context only when every step has succeeded.  After a refusal the context has NO table.
int install_table(pfac_ctx *ctx, const int *d_blob, const int32_t *hdr, size_t n_words, hipStream_t stream) {
    if (hdr[0] != PFAC_BLOB_MAGIC || hdr[1] != PFAC_BLOB_VERSION) return fail(ctx, PFAC_E_ARG, "not a PFAC table image");
    const int width = hdr[2], wbit = hdr[3], num_final = hdr[5], state_num = hdr[6], max_pat_len = hdr[7];
    const int max_row = hdr[8], ht_size = hdr[9];
    if (width < 1 || width > 4096 || (1 << wbit) != width || num_final < 0 || state_num < num_final + 2 ||
        max_row < 1 || ht_size < 1 || max_pat_len < 0 || max_pat_len > HALO_MAX - 1 ||
        (size_t)PFAC_BLOB_HEADER_WORDS + 256 + (size_t)max_row + 2 * (size_t)ht_size + (size_t)num_final > n_words)
        return fail(ctx, PFAC_E_ARG, "inconsistent PFAC table image header");
    if ((int64_t)max_row < ((int64_t)state_num * 256 >> wbit) + 1)
        return fail(ctx, PFAC_E_ARG, "table image: r[] shorter than state_num*256/width+1");
    for (auto &sl : ctx->slots)                             // a scan still in flight reads the tables freed below
        if (sl.pending) { int rc = wait_scan(ctx, sl); if (rc) return rc; }
    ctx->plan = TablePlan();
    ctx->flen.reset(); ctx->fold = PFAC_FOLD_NONE;          // the lengths belong to the old table, and so does the case fold
    ctx->rep_off.reset(); ctx->rep.reset(); ctx->rep_split.reset();       // ... and so do the replacements and their splits
    ctx->gmask.reset();                                     // ... and the state groups
    ctx->sweight.reset();                                   // ... and the state weights
    ctx->spans.reset();                                     // ... and the state spans
    ctx->tok.reset(); ctx->btok.reset();                    // ... and the token ids
    ctx->wp_ids.reset(); ctx->wp_btok.reset();              // ... and the WordPiece ids
    ctx->ug_pieces.reset(); ctx->ug_btok.reset();           // ... and the Unigram pieces
    ctx->bpe_pieces.reset(); ctx->bpe_btok.reset();         // ... and the BPE pieces
    ctx->ru_sptr.reset(); ctx->ru_ent.reset(); ctx->ru_need.reset(); ctx->ru_n = ctx->ru_terms = 0;     // ... and the rules
    ctx->have_table = false; ctx->table_gen++;
    TablePlan P;
    if (int rc = build_plan(ctx, P, d_blob, hdr, stream)) return rc;
    ctx->plan = std::move(P);
    ctx->dense = ctx->plan.knobs.dense == 1 && ctx->plan.lay_d.stage_cap;
    ctx->lag2 = ctx->plan.lag2_ok;
    ctx->have_table = true;
    return PFAC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" {

const char *pfac_last_error(const pfac_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int pfac_device_count(int *n) {
    if (!n) return fail(nullptr, PFAC_E_ARG, "null argument");
    *n = 0;
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; return fail(nullptr, PFAC_E_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    return PFAC_OK;
}

int pfac_ctx_create(int device, int n_streams, pfac_ctx **out) {
    if (!out || n_streams < 1 || n_streams > 64) return fail(nullptr, PFAC_E_ARG, "bad argument to pfac_ctx_create");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(nullptr, PFAC_E_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, PFAC_E_NO_DEVICE, "device index out of range");
    pfac_ctx *ctx = new pfac_ctx();
    ctx->device = device;
    USE_DEVICE(ctx);
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, device));
    ctx->n_cu = prop.multiProcessorCount;
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess) (void)hipGetLastError();
    ctx->tick_ms = 1.0 / (khz > 0 ? khz : 100000);          // (100 MHz where the runtime does not say)
    ctx->event_timing = env_int("PFAC_EVENT_TIMING", 0) != 0;
    ctx->slots.resize(n_streams);
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (auto &s : ctx->slots) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&s.own_stream, hipStreamNonBlocking));
        s.stream = s.own_stream;
        HIP_TRY(ctx, hipHostMalloc((void **)&s.h_ctl, H_CTL_BYTES, hipHostMallocMapped));
        memset(s.h_ctl, 0, H_CTL_BYTES);
        HIP_TRY(ctx, hipHostGetDevicePointer((void **)&s.d_res, s.h_ctl, 0));
        int rc = s.sum.ensure(ctx, nullptr, 2, 2);
        if (rc) return rc;
        if (ctx->event_timing) {
            HIP_TRY(ctx, hipEventCreate(&s.ev0));
            HIP_TRY(ctx, hipEventCreate(&s.ev1));
        }
        HIP_TRY(ctx, hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&s.ev_rd, hipEventDisableTiming));
    }
    *out = ctx;
    return PFAC_OK;
}

void pfac_ctx_destroy(pfac_ctx *ctx) {
    if (!ctx) return;
    DeviceGuard device_guard_(ctx->device);
    if (ctx->clk_n && knob("PFAC_VERBOSE"))
        fprintf(stderr, "pfac: event time - kernel's own clock: mean %.2f us over %llu timed scans\n",
                ctx->clk_diff_ms * 1e3 / (double)ctx->clk_n, (unsigned long long)ctx->clk_n);
    for (auto &s : ctx->slots) {
        if (s.own_stream) (void)hipStreamSynchronize(s.own_stream);
        if (s.h_ctl) (void)hipHostFree(s.h_ctl);
        if (s.ev0) (void)hipEventDestroy(s.ev0);
        if (s.ev1) (void)hipEventDestroy(s.ev1);
        if (s.ev_h2d) (void)hipEventDestroy(s.ev_h2d);
        if (s.ev_rd) (void)hipEventDestroy(s.ev_rd);
        if (s.own_stream) (void)hipStreamDestroy(s.own_stream);
    }
    if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
    // every device buffer of the slots and the context goes with its DevBuf: the streams are idle, the device guard holds
    delete ctx;
}

int pfac_table_upload(pfac_ctx *ctx, const int32_t *blob, size_t n_words) {
    if (!ctx || !blob || n_words < PFAC_BLOB_HEADER_WORDS) return fail(ctx, PFAC_E_ARG, "bad argument to pfac_table_upload");
    std::lock_guard<std::mutex> lk(ctx->mu);
    USE_DEVICE(ctx);
    DevBuf<int> d_blob;
    int rc = d_blob.ensure(ctx, nullptr, n_words, n_words);
    if (rc) return rc;
    hipError_t e = hipMemcpy(d_blob.p, blob, n_words * 4, hipMemcpyHostToDevice);   // master_kernel.cu:365-383
    return e == hipSuccess ? install_table(ctx, d_blob.p, blob, n_words, ctx->slots[0].stream)
                           : fail(ctx, PFAC_E_HIP, std::string("hipMemcpy(table): ") + hipGetErrorString(e));
}

int pfac_table_upload_device(pfac_ctx *ctx, const void *d_blob, size_t n_words, void *stream_handle) {
    if (!ctx || !d_blob || n_words < PFAC_BLOB_HEADER_WORDS) return fail(ctx, PFAC_E_ARG, "bad argument to pfac_table_upload_device");
    std::lock_guard<std::mutex> lk(ctx->mu);
    USE_DEVICE(ctx);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream_handle);
    int32_t hdr[PFAC_BLOB_HEADER_WORDS];
    HIP_TRY(ctx, hipMemcpyAsync(hdr, d_blob, sizeof hdr, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return install_table(ctx, reinterpret_cast<const int *>(d_blob), hdr, n_words, st);
}

int pfac_host_alloc(void **p, size_t n_bytes) {
    if (!p) return fail(nullptr, PFAC_E_ARG, "null argument");
    hipError_t e = hipHostMalloc(p, n_bytes ? n_bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) { *p = nullptr; return fail(nullptr, PFAC_E_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e)); }
    return PFAC_OK;
}
void pfac_host_free(void *p) { if (p) (void)hipHostFree(p); }

int pfac_host_register(void *p, size_t n_bytes) {
    if (!p || !n_bytes) return fail(nullptr, PFAC_E_ARG, "bad argument to pfac_host_register");
    hipError_t e = hipHostRegister(p, n_bytes, hipHostRegisterPortable);     // (usable from every device's context)
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, PFAC_E_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
    return PFAC_OK;
}
int pfac_host_unregister(void *p) {
    if (!p) return fail(nullptr, PFAC_E_ARG, "null argument");
    hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, PFAC_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return PFAC_OK;
}

int pfac_slot_reserve(pfac_ctx *ctx, int slot, uint64_t input_bytes, uint64_t record_capacity) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    USE_DEVICE(ctx);
    Slot &s = ctx->slots[slot];
    // Replacing a buffer the slot already has: whatever the slot's stream and the copy stream still do with the old one
    // finishes first (a pending scan writes the heap and reads the input), and the new, uninitialised buffer holds no
    // scan -- the slot is back to "no finished scan", so nothing reads it as if it held the last one.
    if ((input_bytes > s.input.cap && s.input.p) || (record_capacity > s.records.cap && s.records.p)) {
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        if (s.pending) { rc = wait_scan(ctx, s); if (rc) return rc; }
        if (s.h2d_issued) HIP_TRY(ctx, hipEventSynchronize(s.ev_h2d));
        s.scanned = s.pending = false;
    }
    rc = s.input.ensure(ctx, s.stream, input_bytes, align_up(input_bytes, WTILE) + HALO_MAX + 256);
    if (rc) return rc;
    return s.records.ensure(ctx, s.stream, record_capacity, record_capacity);
}

void *pfac_slot_input(pfac_ctx *ctx, int slot) { return check_slot(ctx, slot) ? nullptr : ctx->slots[slot].input.p; }
void *pfac_slot_records(pfac_ctx *ctx, int slot) { return check_slot(ctx, slot) ? nullptr : ctx->slots[slot].records.p; }
void *pfac_slot_stream(pfac_ctx *ctx, int slot) { return check_slot(ctx, slot) ? nullptr : (void *)ctx->slots[slot].stream; }

int pfac_slot_set_stream(pfac_ctx *ctx, int slot, void *stream_handle) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    hipStream_t ns = stream_handle ? reinterpret_cast<hipStream_t>(stream_handle) : s.own_stream;
    // what the slot still has queued on the old stream finishes first: a scan in flight zeroes the next scan's control
    // words, and the writes of a pass (a selection, say) are asynchronous -- the next pass, on the new stream, reads them
    if (ns != s.stream) {
        USE_DEVICE(ctx);
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        if (s.pending) { rc = wait_scan(ctx, s); if (rc) return rc; }   // (the scan itself: it is not left behind on the old stream)
    }
    s.stream = ns;
    return PFAC_OK;
}

int pfac_slot_h2d(pfac_ctx *ctx, int slot, const void *host, uint64_t n_bytes, uint64_t dst_offset) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!host || dst_offset + n_bytes > s.input.cap) return fail(ctx, PFAC_E_ARG, "pfac_slot_h2d: range exceeds the reserved input buffer");
    USE_DEVICE(ctx);
    // on the context's copy stream, behind whatever the slot's stream still does with the buffer: its last scan reads it,
    // and so do kernels queued behind the scan by calls that have already returned (the write kernels of the replace passes,
    // of the split and of the gather). ev_rd, recorded here, is behind all of them: a stream swap leaves no scan behind on
    // the old stream (pfac_slot_set_stream waits for it). The slot's stream then waits for the copy: same ordering as a
    // copy on the slot's stream, without the gaps
    HIP_TRY(ctx, hipEventRecord(s.ev_rd, s.stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, s.ev_rd, 0));
    HIP_TRY(ctx, hipMemcpyAsync(s.input.p + dst_offset, host, n_bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    HIP_TRY(ctx, hipEventRecord(s.ev_h2d, ctx->copy_stream));
    HIP_TRY(ctx, hipStreamWaitEvent(s.stream, s.ev_h2d, 0));
    s.h2d_issued = true;
    return PFAC_OK;
}

int pfac_slot_h2d_done(pfac_ctx *ctx, int slot) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    USE_DEVICE(ctx);
    const hipError_t e = hipEventQuery(ctx->slots[slot].ev_h2d);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return fail(ctx, PFAC_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
}

int pfac_slot_h2d_wait(pfac_ctx *ctx, int slot) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    USE_DEVICE(ctx);
    HIP_TRY(ctx, hipEventSynchronize(ctx->slots[slot].ev_h2d));   // (an event never recorded counts as complete)
    return PFAC_OK;
}

int pfac_scan_async(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_owned, uint64_t n_avail,
                    void *d_records, uint64_t capacity) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_scan_async before a table upload");
    Slot &s = ctx->slots[slot];
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    if (!d_records) { d_records = s.records.p; capacity = s.records.cap; }
    if (!in) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: no input buffer");
    if (((uintptr_t)in & 15) != 0) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: input pointer must be 16-byte aligned");
    if (n_owned > n_avail || n_owned > (1ull << 32)) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: need n_owned <= n_avail and n_owned <= 2^32");
    if (!d_input && n_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: n_avail exceeds the reserved input buffer");
    if (((uintptr_t)d_records & 15) != 0) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: record buffer must be 16-byte aligned");
    if (!d_records && capacity) return fail(ctx, PFAC_E_ARG, "pfac_scan_async: no record buffer");
    USE_DEVICE(ctx);
    const uint64_t n_tiles = (n_owned + WTILE - 1) / WTILE;
    if (s.pending) HIP_TRY(ctx, hipStreamSynchronize(s.stream));   // the previous scan of this slot still owns h_ctl
    s.last_cap = capacity;
    s.scanned = true;
    s.pending = true;
    for (int i = 0; i < 8; i++) s.h_ctl[i] = 0;        // result words and H_DONE (the kernel writes them through the host mapping)
    s.h_ctl[H_T0] = s.h_ctl[H_T0 + 1] = s.h_ctl[H_T1] = s.h_ctl[H_T1 + 1] = 0;
    // wait_scan polls for 2 ms + what the owned bytes take at 50 GB/s (a hundred times the headline scan, six times the
    // dictionary's) before it asks the stream instead
    s.spin_ms = 2.0 + (double)n_owned / 50e6;
    // staging mode of this launch (see pfac_scan_finish for the adaptation)
    const TablePlan &P = ctx->plan;
    const bool dense = ctx->run_dense();
    const StageLayout &L = ctx->layout(dense);
    const int wpb = L.waves_per_block;
    s.last_dense = dense;
    s.last_tiles = n_tiles;
    s.last_owned = n_owned;
    s.last_avail = n_avail;
    s.scan_seq++;
    s.rf_done = false;
    s.last_table = ctx->table_gen;
    s.last_rec_bytes = (int)P.base.rec_bytes;
    s.last_records = d_records;
    // The control header (ticket counters, flags, heap cursor) must start at zero.  The slot has two: every scan
    // zeroes, in its own prologue, the other one for the scan after it, so back-to-back scans need no memset.
    rc = ensure_ctl(ctx, s);
    if (rc) return rc;
    rc = s.tile_index.ensure(ctx, s.stream, n_tiles + 1, quarter_more(n_tiles + 1));
    if (rc) return rc;
    const uint64_t n_batches = (n_tiles + wpb - 2) / (wpb - 1);
    unsigned *const cur = s.d_ctlbuf[s.flip], *const nxt = s.d_ctlbuf[1 - s.flip];
    if (n_tiles > 0 && !s.clean[s.flip]) HIP_TRY(ctx, hipMemsetAsync(cur, 0, CTL_REGION, s.stream));
    if (n_tiles > 0) {
        ScanArgs a = P.base;                   // what the table fixes; below, what this launch adds
        a.in = in; a.n_owned = n_owned; a.n_avail = n_avail;
        a.out = d_records; a.out_cap = capacity;
        a.tile_index = s.tile_index.p;
        a.pw_bytes = L.pw_bytes; a.stage_cap = L.stage_cap; a.nbuf = (unsigned)L.nbuf;
        a.dense2 = dense && P.dense2 ? 1 : 0;
        if (a.dense2) {
            a.stage_cap = 0;                   // (its LDS carve has no staging buffer: a tile it gives up on is counted, then written directly)
            const size_t words = (size_t)P.grid_blocks * (size_t)(wpb - 1) * a.d2log_cap;
            rc = s.d2log.ensure(ctx, s.stream, words, words);
            if (rc) return rc;
            a.d2log = s.d2log.p;
        }
        a.n_tiles = (unsigned)n_tiles; a.ctl = cur; a.res = s.d_res;
        a.zero_next = reinterpret_cast<uint4 *>(nxt); a.zero_vec = (unsigned)(CTL_REGION / 16);
#ifdef PFAC_TRACE_BUILD
        if (!P.knobs.trace_file.empty()) {
            rc = s.dbg.ensure(ctx, s.stream, 8 * 64 * 32, 8 * 64 * 32);
            if (rc) return rc;
            HIP_TRY(ctx, hipMemsetAsync(s.dbg.p, 0, 8 * 64 * 32 * 8, s.stream));
            a.dbg = s.dbg.p;
        }
#endif
        const uint64_t grid = std::min<uint64_t>((uint64_t)P.grid_blocks, n_batches);
        a.ticket_ways = grid < TICKET_WAYS ? (unsigned)grid : TICKET_WAYS;
        if (P.knobs.ticket_ways >= 1 && P.knobs.ticket_ways < a.ticket_ways) a.ticket_ways = P.knobs.ticket_ways;
        // heap chunk: 1/32 of an even share of the record array per workgroup -- the current and the spare chunk of
        // every workgroup can stay unfilled at the end, i.e. at most 1/16 of the capacity; record arrays too small for
        // chunks of 1024 records get exact allocations (one atomic per batch)
        uint64_t chunk = (capacity / (32 * grid)) & ~7ull;        // (a multiple of 8 records: see the placement)
        if (chunk > (1u << 22)) chunk = 1u << 22;
        a.chunk = (chunk >= 1024 && !dense) ? (unsigned)chunk : 0u;      // (dense mode: every tile takes its own space)
        void *kargs[] = {&a};
        const unsigned fold = ctx->fold == PFAC_FOLD_ASCII ? 1u : 0u;       // the mode of THIS launch: its kernel
        // A plain dispatch: no completion signal, no timestamps (a dispatch that carries them makes the command processor
        // retire the kernel, fence, write both and signal before it looks at the next packet).  Completion is the H_DONE
        // word and the time is the kernel's own.  PFAC_EVENT_TIMING: both events ride on the dispatch itself (null otherwise).
        HIP_TRY(ctx, hipExtLaunchKernel(P.kernel_of(dense, ctx->lag2, fold), dim3((unsigned)grid), dim3(WAVE * wpb), kargs,
                                        (size_t)L.lds_bytes, s.stream, s.ev0, s.ev1, 0));
        s.clean[s.flip] = false;               // used by this scan
        s.clean[1 - s.flip] = true;            // zeroed by this scan
        s.flip = 1 - s.flip;
    }
    if (n_tiles == 0) {                                // nothing launched: complete, in no time
        if (ctx->event_timing) HIP_TRY(ctx, hipEventRecord(s.ev1, s.stream));
        __atomic_store_n(s.h_ctl + H_DONE, 1u, __ATOMIC_RELEASE);
    }
    return PFAC_OK;
}

int pfac_scan_finish(pfac_ctx *ctx, int slot, uint64_t *n_matches) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!s.scanned) return fail(ctx, PFAC_E_STATE, "pfac_scan_finish without a scan");
    USE_DEVICE(ctx);
    rc = wait_scan(ctx, s);
    if (rc) return rc;
    // (an empty scan launched nothing that ran behind the slot's uploads: a caller releases their host buffers now)
    if (s.last_tiles == 0 && s.h2d_issued) HIP_TRY(ctx, hipEventSynchronize(s.ev_h2d));
    s.pending = false;
    const uint64_t total = host_u64(s, H_MATCHES);
    s.last_total = total;
    s.last_used = host_u64(s, H_USED);
    if (n_matches) *n_matches = total;
#ifdef PFAC_TRACE_BUILD
    if (s.dbg.p && !ctx->plan.knobs.trace_file.empty()) {
        std::vector<unsigned long long> h(8 * 64 * 32);
        if (hipMemcpy(h.data(), s.dbg.p, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(ctx->plan.knobs.trace_file.c_str(), "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
        }
    }
#endif
    if (s.h_ctl[2] != 0) {
        s.clean[0] = s.clean[1] = false;       // whatever state the control headers are in: zero them before the next scan
        return fail(ctx, PFAC_E_INTERNAL, "scan kernel reported a timeout (flags " + std::to_string(s.h_ctl[2]) +
                                          ": 4 arrivals, 8 record base, 16 batch ring)");
    }
    // Staging mode for the NEXT scans of this context: when more than a quarter of the tiles held more matches
    // than the two-buffer staging area takes, go dense (one big buffer, emitted at once, no second walk); go back
    // when fewer than 1/16 do.  PFAC_DENSE=0/1 pins the mode.  Likewise between the three- and the two-buffer layout,
    // on the tiles above the (smaller) three-buffer capacity: 1/16 of the tiles walked twice cost what the earlier
    // emission gains.  PFAC_LAG=1/2 pins that.
    if (ctx->plan.knobs.dense < 0 && ctx->plan.lay_d.stage_cap && s.last_tiles >= 64) {
        const uint64_t ovf = s.h_ctl[3];
        if (!ctx->dense && ovf * 4 > s.last_tiles) ctx->dense = true;
        else if (ctx->dense && ovf * 16 < s.last_tiles) ctx->dense = false;
    }
    if (ctx->plan.lag2_ok && ctx->plan.knobs.lag != 1 && ctx->plan.knobs.lag != 2 && s.last_tiles >= 64) {
        const uint64_t ovf2 = s.h_ctl[6];
        if (ctx->lag2 && ovf2 * 16 > s.last_tiles) ctx->lag2 = false;
        else if (!ctx->lag2 && ovf2 * 64 < s.last_tiles) ctx->lag2 = true;
    }
    if (s.last_used > s.last_cap)
        return fail(ctx, PFAC_E_OVERFLOW, "record array too small: " + std::to_string(total) + " matches need " +
                                              std::to_string(s.last_used) + " records of capacity (pfac_scan_capacity_hint)");
    return PFAC_OK;
}

int pfac_scan_elapsed_ms(pfac_ctx *ctx, int slot, float *ms) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!ms) return fail(ctx, PFAC_E_ARG, "null argument");
    Slot &s = ctx->slots[slot];
    if (!s.scanned) return fail(ctx, PFAC_E_STATE, "no scan to time");
    USE_DEVICE(ctx);
    rc = wait_scan(ctx, s);
    if (rc) return rc;
    if (s.last_tiles == 0) *ms = 0.0f;
    else if (ctx->event_timing) {
        HIP_TRY(ctx, hipEventElapsedTime(ms, s.ev0, s.ev1));
        ctx->clk_diff_ms += *ms - (double)(host_u64(s, H_T1) - host_u64(s, H_T0)) * ctx->tick_ms;   // the two clocks, same launch
        ctx->clk_n++;
    }
    else *ms = (float)((double)(host_u64(s, H_T1) - host_u64(s, H_T0)) * ctx->tick_ms);
    return PFAC_OK;
}

// Records [first, first+n) of the slot's last scan, in (position, pattern length) order -> pfac_record at d_out
// (device), on the slot's stream: prefix over the tile index, then a copy out of the heap.
static int expand_records(pfac_ctx *ctx, Slot &s, const void *src, uint64_t first, uint64_t n, pfac_record *d_out) {
    // records that do not exist, or that the last scan could not write, are never delivered as if they did: the copy
    // kernel skips them and the caller would read whatever its buffer held before
    if (s.pending) return fail(ctx, PFAC_E_STATE, "records requested before pfac_scan_finish");
    if (!in_window(first, n, s.last_total)) return fail(ctx, PFAC_E_ARG, "records [first, first + n) exceed the scan's match count");
    int rc = last_scan_usable(ctx, s, "", SCAN_FITS);
    if (rc) return rc;
    if (n == 0 || s.last_tiles == 0) return PFAC_OK;
    const unsigned n_groups = (unsigned)((s.last_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, n_groups);
    if (rc) return rc;
    const unsigned gblocks = (n_groups + 3) / 4;           // four waves (groups) per 256-thread block
    hipLaunchKernelGGL(pfac_tix_group_sum_kernel, dim3(gblocks), dim3(256), 0, s.stream, s.tile_index.p,
                       (unsigned long long)s.last_tiles, s.gsum.p, n_groups);
    hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
    auto ek = by_width(s.last_rec_bytes, [](auto w) { return pfac_expand_kernel<w()>; });
    hipLaunchKernelGGL(ek, dim3(gblocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)s.last_tiles,
                       s.gsum.p, n_groups, (unsigned long long)s.last_cap, (unsigned long long)first, (unsigned long long)n, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return PFAC_OK;
}

int pfac_scan_format(pfac_ctx *ctx, int slot, int *record_bytes, uint64_t *n_tiles, uint64_t *used) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!s.scanned) return fail(ctx, PFAC_E_STATE, "no scan yet");
    if (record_bytes) *record_bytes = s.last_rec_bytes;
    if (n_tiles) *n_tiles = s.last_tiles;
    if (used) *used = s.last_used;
    return PFAC_OK;
}

int pfac_scan_capacity_hint(pfac_ctx *ctx, int slot, uint64_t *capacity) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!s.scanned || !capacity) return fail(ctx, PFAC_E_STATE, "pfac_scan_capacity_hint: no finished scan");
    // what the finished scan used (+ 1/8: a larger array means larger chunks, i.e. more unfilled space at the end)
    // and a floor from the match count
    const uint64_t a = s.last_used + s.last_used / 8, b = s.last_total + s.last_total / 4;
    *capacity = (a > b ? a : b) + 65536;
    return PFAC_OK;
}

int pfac_records_expand(pfac_ctx *ctx, int slot, const void *d_records, uint64_t first, uint64_t n, pfac_record *d_out) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    if (!s.scanned) return fail(ctx, PFAC_E_STATE, "pfac_records_expand without a scan");
    if (!src || (!d_out && n) || ((uintptr_t)d_out & 7)) return fail(ctx, PFAC_E_ARG, "pfac_records_expand: bad buffer");
    USE_DEVICE(ctx);
    return expand_records(ctx, s, src, first, n, d_out);
}

int pfac_records_d2h(pfac_ctx *ctx, int slot, const void *d_records, pfac_record *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    if (n == 0) return PFAC_OK;
    if (!s.scanned) return fail(ctx, PFAC_E_STATE, "pfac_records_d2h without a scan");
    if (!src || !host) return fail(ctx, PFAC_E_ARG, "pfac_records_d2h: null buffer");
    USE_DEVICE(ctx);
    rc = s.wide.ensure(ctx, s.stream, n, n);
    if (rc) return rc;
    rc = expand_records(ctx, s, src, first, n, s.wide.p);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(host, s.wide.p, n * sizeof(pfac_record), hipMemcpyDeviceToHost, s.stream));
    return PFAC_OK;
}

int pfac_records_d2h_packed(pfac_ctx *ctx, int slot, const void *d_records, void *host_words, uint64_t n_words,
                            uint64_t *host_tile_index) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    if (!s.scanned || s.last_rec_bytes == 8) return fail(ctx, PFAC_E_STATE, "pfac_records_d2h_packed: the slot's last scan did not produce compact records");
    if (!src || (!host_words && n_words) || !host_tile_index) return fail(ctx, PFAC_E_ARG, "pfac_records_d2h_packed: null buffer");
    if (n_words > s.last_cap) return fail(ctx, PFAC_E_ARG, "pfac_records_d2h_packed: more words than the record array holds");
    USE_DEVICE(ctx);
    if (n_words) HIP_TRY(ctx, hipMemcpyAsync(host_words, src, n_words * (uint64_t)s.last_rec_bytes, hipMemcpyDeviceToHost, s.stream));
    if (s.last_tiles) HIP_TRY(ctx, hipMemcpyAsync(host_tile_index, s.tile_index.p, s.last_tiles * 8, hipMemcpyDeviceToHost, s.stream));
    return PFAC_OK;
}

int pfac_records_packed_device(pfac_ctx *ctx, int slot, const void *d_records, void *d_words_out, uint64_t n_words,
                               uint64_t *d_tile_index_out) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    if (!s.scanned || s.pending || s.last_rec_bytes == 8) return fail(ctx, PFAC_E_STATE, "pfac_records_packed_device: the slot's last finished scan did not produce compact records");
    rc = last_scan_usable(ctx, s, "", SCAN_FITS);
    if (rc) return rc;
    if (!d_tile_index_out || (d_words_out && !src)) return fail(ctx, PFAC_E_ARG, "pfac_records_packed_device: null buffer");
    if (n_words > s.last_cap) return fail(ctx, PFAC_E_ARG, "pfac_records_packed_device: more words than the record array holds");
    USE_DEVICE(ctx);
    if (d_words_out && n_words && d_words_out != src)
        HIP_TRY(ctx, hipMemcpyAsync(d_words_out, src, n_words * (uint64_t)s.last_rec_bytes, hipMemcpyDeviceToDevice, s.stream));
    if (s.last_tiles) HIP_TRY(ctx, hipMemcpyAsync(d_tile_index_out, s.tile_index.p, s.last_tiles * 8, hipMemcpyDeviceToDevice, s.stream));
    return PFAC_OK;
}

int pfac_emit_text_device(pfac_ctx *ctx, int slot, const void *d_records, uint64_t base, uint64_t *n_bytes) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_bytes) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_bytes = 0;
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "no table uploaded");
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    rc = last_scan_usable(ctx, s, "pfac_emit_text_device", SCAN_FINISHED | SCAN_IDMAP | SCAN_FITS);
    if (rc) return rc;
    if (base + (1ull << 32) >= 1000000000000000000ull) return fail(ctx, PFAC_E_ARG, "pfac_emit_text_device: positions must stay below 10^18");
    s.text_bytes = 0;
    if (s.last_total == 0 || s.last_tiles == 0) return PFAC_OK;
    if (!src) return fail(ctx, PFAC_E_ARG, "null record buffer");
    USE_DEVICE(ctx);
    const unsigned n_groups = (unsigned)((s.last_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, n_groups);
    if (rc) return rc;
    const unsigned gblocks = (n_groups + 3) / 4;           // four waves (groups of 64 tiles) per 256-thread block
    auto sk = by_width(s.last_rec_bytes, [](auto w) { return pfac_text_size_kernel<w()>; });
    hipLaunchKernelGGL(sk, dim3(gblocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)s.last_tiles,
                       (unsigned long long)s.last_cap, (unsigned long long)base, ctx->plan.d_idmap, s.gsum.p, n_groups);
    hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, s.gsum.p + n_groups, 8, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    rc = s.text.ensure(ctx, s.stream, total + 32, total + total / 8 + 4096);
    if (rc) return rc;
    auto fk = by_width(s.last_rec_bytes, [](auto w) { return pfac_text_format_kernel<w()>; });
    hipLaunchKernelGGL(fk, dim3(gblocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)s.last_tiles,
                       (unsigned long long)s.last_cap, (unsigned long long)base, ctx->plan.d_idmap, s.gsum.p, n_groups, s.text.p);
    HIP_TRY(ctx, hipGetLastError());
    s.text_bytes = total;
    *n_bytes = total;
    return PFAC_OK;
}

int pfac_text_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    if (!in_window(first, n, s.text_bytes)) return fail(ctx, PFAC_E_ARG, "pfac_text_d2h: range exceeds the text of the slot's last pfac_emit_text_device");
    if (n == 0) return PFAC_OK;
    if (!host) return fail(ctx, PFAC_E_ARG, "null buffer");
    USE_DEVICE(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(host, s.text.p + first, n, hipMemcpyDeviceToHost, s.stream));
    return PFAC_OK;
}

void *pfac_slot_text(pfac_ctx *ctx, int slot) { return check_slot(ctx, slot) ? nullptr : ctx->slots[slot].text.p; }

int pfac_slot_sync(pfac_ctx *ctx, int slot) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    USE_DEVICE(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->slots[slot].stream));
    if (ctx->slots[slot].h2d_issued) HIP_TRY(ctx, hipEventSynchronize(ctx->slots[slot].ev_h2d));   // (a copy nothing on the stream has waited for yet)
    return PFAC_OK;
}

int pfac_records_checksum(pfac_ctx *ctx, int slot, const void *d_records, uint64_t n, uint64_t base, uint64_t *checksum) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!checksum) return fail(ctx, PFAC_E_ARG, "null argument");
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "no table uploaded");
    Slot &s = ctx->slots[slot];
    const void *src = d_records ? d_records : s.records.p;
    rc = n ? last_scan_usable(ctx, s, "pfac_records_checksum", SCAN_FINISHED | SCAN_IDMAP | SCAN_FITS) : PFAC_OK;
    if (rc) return rc;
    if (!src && n) return fail(ctx, PFAC_E_ARG, "null record buffer");
    USE_DEVICE(ctx);
    HIP_TRY(ctx, hipMemsetAsync(s.sum.p, 0, 16, s.stream));
    if (n && s.last_tiles) {
        auto ck = by_width(s.last_rec_bytes, [](auto w) { return pfac_checksum_kernel<w()>; });
        hipLaunchKernelGGL(ck, dim3(1024), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)s.last_tiles,
                           (unsigned long long)s.last_cap, (unsigned long long)base, ctx->plan.d_idmap, s.sum.p);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + H_CHECKSUM, s.sum.p, 8, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    *checksum = host_u64(s, H_CHECKSUM);
    return PFAC_OK;
}

}  // extern "C"

namespace {

using CountKernel = void (*)(const void *, const unsigned long long *, unsigned long long, unsigned long long, unsigned, unsigned,
                             unsigned long long *, unsigned long long *);

// pfac_records_count_states (the heap `heap` through the tile index) and, with is_sel, pfac_selection_count_states
// (the n_sel records of `sel`; check_sel: it is the caller's), behind their checks of the scan's and the selection's
// state: the arguments, then the histogram.  Nothing is written before every check has passed.
int count_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *heap, bool is_sel, const pfac_record *sel, uint64_t n_sel,
              bool check_sel, uint64_t *d_counts, uint64_t n_states, uint32_t flags, uint64_t *n_counted) {
    if (flags > PFAC_COUNT_ACCUMULATE) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 or PFAC_COUNT_ACCUMULATE");
    if (n_states != (uint64_t)ctx->plan.base.num_final)
        return fail(ctx, PFAC_E_ARG, fn + ": n_states must be num_final of the uploaded table (" + std::to_string(ctx->plan.base.num_final) + ")");
    if ((uintptr_t)d_counts & 7) return fail(ctx, PFAC_E_ARG, fn + ": d_counts must be 8-byte aligned");
    const bool own = d_counts == nullptr, acc = (flags & PFAC_COUNT_ACCUMULATE) != 0;
    if (own && acc && s.cnt.done && s.cnt_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's counts belong to an earlier table; they cannot be added to");
    const uint64_t expect = is_sel ? n_sel : s.last_total;
    const uint64_t n_items = is_sel ? (n_sel + WAVE - 1) / WAVE : s.last_tiles;
    if (!(is_sel ? (const void *)sel : heap) && n_items) return fail(ctx, PFAC_E_ARG, "null record buffer");
    USE_DEVICE(ctx);
    int rc = ensure_gsum(ctx, s, 1);                        // the records counted, the selection check's flag
    if (rc) return rc;
    unsigned long long *res = s.gsum.p;
    const unsigned ns = (unsigned)n_states;
    if (check_sel && n_sel) {                               // a caller's selection: judged before a counter changes
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        const unsigned blocks = (unsigned)std::min<uint64_t>((n_sel + 255) / 256, 1024);
        hipLaunchKernelGGL(pfac_sel_check_kernel, dim3(blocks), dim3(256), 0, s.stream, sel, (unsigned long long)n_sel, ns, res + 1);
        rc = pass_words(ctx, s, res + 1, 1, H_PASS1);
        if (rc) return rc;
        if (host_u64(s, H_PASS1)) return fail(ctx, PFAC_E_ARG, fn + ": d_sel is not the selection of this scan and table");
    }
    unsigned long long *dst;
    const bool zero = !acc || (own && !s.cnt.done);
    rc = s.cnt.bind(ctx, s.stream, d_counts, std::max<uint64_t>(n_states, 1), std::max<uint64_t>(n_states, 1), &dst);
    if (rc) { s.cnt.invalidate(); return rc; }             // (it grows only where the counts start from zero)
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 8, s.stream));
    if (zero && n_states) HIP_TRY(ctx, hipMemsetAsync(dst, 0, n_states * 8, s.stream));
    if (n_items && n_states) {
        // a direct table while the states fit it, else the cache
        const bool direct = ns <= (ctx->plan.knobs.count_bins ? std::min(ctx->plan.knobs.count_bins, COUNT_DIRECT_MAX) : COUNT_DIRECT_MAX);
        const unsigned bins = ctx->plan.knobs.count_bins ? ctx->plan.knobs.count_bins : COUNT_CACHE_SLOTS;
        const size_t lds = direct ? (size_t)ns * 4 : (size_t)bins * 8;
        // The grid.  Direct table: workgroups of four waves, as many per CU as their LDS lets be resident, eight at
        // most (the loads of 32 waves hide the heap's latency).  Cache: ONE workgroup of sixteen waves per CU with
        // most of its LDS -- every workgroup flushes the slots it claimed and misses what it could not claim, so
        // more, smaller workgroups over the same records mean more atomics in memory (both measured: DESIGN.md,
        // section 12).  Never fewer than two workgroups (the bound of a workgroup's 32-bit partials, see the
        // kernel), never more than there is work for.
        const unsigned per_cu = direct ? (unsigned)std::min<size_t>(8, LDS_TOTAL / std::max<size_t>(lds, 1)) : 1u;
        const unsigned threads = ctx->plan.knobs.count_threads ? ctx->plan.knobs.count_threads : (unsigned)(direct ? COUNT_THREADS : COUNT_THREADS_MAX);
        const uint64_t wanted = (n_items + threads / WAVE - 1) / (threads / WAVE);
        unsigned grid = (unsigned)std::min<uint64_t>(wanted, (uint64_t)per_cu * (unsigned)std::max(ctx->n_cu, 1));
        if (ctx->plan.knobs.count_grid) grid = ctx->plan.knobs.count_grid;
        if (grid < 2) grid = 2;
        CountKernel k = direct ? pfac_count_kernel<0, true> : pfac_count_kernel<0, false>;
        if (!is_sel) k = by_width(s.last_rec_bytes, [direct](auto w) -> CountKernel { return direct ? pfac_count_kernel<w(), true> : pfac_count_kernel<w(), false>; });
        if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, s.stream, is_sel ? (const void *)sel : heap,
                           is_sel ? (const unsigned long long *)nullptr : s.tile_index.p, (unsigned long long)n_items,
                           (unsigned long long)(is_sel ? n_sel : s.last_cap), ns, bins, dst, res);
    }
    rc = pass_words(ctx, s, res, 1);
    if (rc) return rc;
    const uint64_t total = host_u64(s, H_PASS);
    if (own) {
        s.cnt.commit(n_states, true);
        s.cnt_table = ctx->table_gen;
    }
    *n_counted = total;
    if (total != expect)
        return fail(ctx, PFAC_E_INTERNAL, fn + ": counted " + std::to_string(total) + " records of " + std::to_string(expect) +
                                              " (a final state at or past n_states)");
    return PFAC_OK;
}

}  // namespace

extern "C" {

int pfac_records_count_states(pfac_ctx *ctx, int slot, const void *d_records, uint64_t *d_counts, uint64_t n_states,
                              uint32_t flags, uint64_t *n_counted) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_counted) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_counted = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_records_count_states";
    rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_TABLE | SCAN_FITS);
    if (rc) return rc;
    const void *heap = d_records ? d_records : (const void *)s.records.p;
    if (s.last_tiles && heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    return count_run(ctx, s, fn, heap, false, nullptr, 0, false, d_counts, n_states, flags, n_counted);
}

int pfac_selection_count_states(pfac_ctx *ctx, int slot, const pfac_record *d_sel, uint64_t *d_counts, uint64_t n_states,
                                uint32_t flags, uint64_t *n_counted) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_counted) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_counted = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_selection_count_states";
    // the rules of pfac_replace_leftmost_longest's d_sel
    if (!s.scanned || s.pending || !s.ll_out.done || s.ll_seq != s.scan_seq)
        return fail(ctx, PFAC_E_STATE, fn + " needs a leftmost-longest selection since the slot's last scan");
    if (!ctx->have_table || s.last_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
    const pfac_record *sel;
    rc = s.ll_out.consume(ctx, fn, "selection (d_sel)", d_sel, ANY_N, &sel);
    if (rc) return rc;
    if ((uintptr_t)d_sel & 7) return fail(ctx, PFAC_E_ARG, fn + ": d_sel must be 8-byte aligned");
    return count_run(ctx, s, fn, nullptr, true, sel, s.ll_out.n, d_sel != nullptr, d_counts, n_states, flags, n_counted);
}

int pfac_state_counts_d2h(pfac_ctx *ctx, int slot, uint64_t *host_counts) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.cnt, "pfac_state_counts_d2h", "slot-owned count (pfac_records_count_states with d_counts NULL)", host_counts, 0, s.cnt.n);
}

int pfac_table_set_final_lengths(pfac_ctx *ctx, const int32_t *len, size_t n) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_set_final_lengths before a table upload");
    if (n != (size_t)ctx->plan.base.num_final || (!len && n)) return fail(ctx, PFAC_E_ARG, "pfac_table_set_final_lengths: need num_final lengths");
    std::vector<short> h(n ? n : 1, (short)-1);
    for (size_t i = 0; i < n; i++) {
        if (len[i] != -1 && (len[i] < 1 || len[i] > 1024))
            return fail(ctx, PFAC_E_ARG, "pfac_table_set_final_lengths: a length outside -1, 1..1024 (final state " + std::to_string(i) + ")");
        h[i] = (short)len[i];
    }
    USE_DEVICE(ctx);
    int rc = ctx->flen.ensure(ctx, nullptr, h.size(), h.size());
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->flen.p, h.data(), h.size() * sizeof(short), hipMemcpyHostToDevice));
    return PFAC_OK;
}

int pfac_table_set_case_fold(pfac_ctx *ctx, uint32_t mode) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_set_case_fold before a table upload");
    if (mode != PFAC_FOLD_NONE && mode != PFAC_FOLD_ASCII)
        return fail(ctx, PFAC_E_ARG, "pfac_table_set_case_fold: mode must be PFAC_FOLD_NONE or PFAC_FOLD_ASCII");
    ctx->fold = mode;                  // read by the next pfac_scan_async: it chooses the kernel a launch runs, so a scan
                                       // already queued keeps the one it was launched with
    return PFAC_OK;
}

int pfac_table_case_fold(pfac_ctx *ctx, uint32_t *mode) {
    if (!ctx || !mode) return fail(ctx, PFAC_E_ARG, "pfac_table_case_fold: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_case_fold before a table upload");
    *mode = ctx->fold;
    return PFAC_OK;
}

int pfac_slot_doc_offsets(pfac_ctx *ctx, int slot, const uint64_t *host_offsets, uint64_t n_docs) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!host_offsets || n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, "pfac_slot_doc_offsets: need n_docs + 1 offsets, n_docs < 2^32");
    Slot &s = ctx->slots[slot];
    USE_DEVICE(ctx);
    s.doc.invalidate();
    rc = ensure_docs(ctx, s, s.doc.buf, n_docs);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(s.doc.buf.p, host_offsets, (n_docs + 1) * 8, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));        // (the caller's array may go once this returns)
    s.doc.commit(n_docs + 1, true);
    s.doc_gen++;
    return PFAC_OK;
}

int pfac_slot_doc_offsets_split(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, int delimiter,
                                uint64_t *n_docs, uint64_t *tail_start) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_docs || !tail_start) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_docs = *tail_start = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_slot_doc_offsets_split";
    if (delimiter < 0 || delimiter > 255) return fail(ctx, PFAC_E_ARG, fn + ": the delimiter must be a byte value, 0..255");
    if (n_bytes > (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_bytes must be at most 2^32");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    if ((uintptr_t)in & 15) return fail(ctx, PFAC_E_ARG, fn + ": d_input must be 16-byte aligned");
    if (!d_input && n_bytes > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": n_bytes exceeds the slot's input buffer");
    USE_DEVICE(ctx);
    const uint64_t n_tiles = (n_bytes + WTILE - 1) / WTILE;
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    uint64_t total = 0, tail = 0;                            // delimiters, and the end of the last one
    const unsigned x4 = (unsigned)delimiter * 0x01010101u;
    const unsigned tblocks = (unsigned)std::min<uint64_t>((n_tiles + 3) / 4, 2048);
    if (n_groups) {
        rc = ensure_gsum(ctx, s, 2 * n_groups + 2);          // group prefixes, the total, the groups' last ends, the two results
        if (rc) return rc;
        rc = s.sp_tile.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (rc) return rc;
        unsigned long long *glast = s.gsum.p + n_groups + 1, *res = glast + n_groups;
        hipLaunchKernelGGL(pfac_split_count_kernel, dim3(tblocks), dim3(256), 0, s.stream, in, (unsigned long long)n_bytes,
                           (unsigned long long)n_tiles, x4, s.sp_tile.p);
        hipLaunchKernelGGL(pfac_split_group_kernel, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, s.sp_tile.p,
                           (unsigned long long)n_tiles, s.gsum.p, glast, n_groups);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
        hipLaunchKernelGGL(pfac_split_ends_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, glast, n_groups, res);
        rc = pass_words(ctx, s, res, 2);
        if (rc) return rc;
        total = host_u64(s, H_PASS);
        tail = host_u64(s, H_PASS1);
    }
    const uint64_t docs = total + (tail != n_bytes ? 1 : 0);
    if (docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": 2^32 documents (every byte is a delimiter); n_docs must be below 2^32");
    // the new offsets go into a buffer of their own where the old one is too small: a failure up to here, the allocation
    // included, leaves the slot's offsets as they were
    if (docs + 1 > s.doc.buf.cap) {
        DevBuf<unsigned long long> grown;
        rc = ensure_docs(ctx, s, grown, docs);
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));        // (nothing queued still reads the old one)
        s.doc.buf = std::move(grown);
    }
    if (n_groups) {
        hipLaunchKernelGGL(pfac_split_write_kernel, dim3(tblocks), dim3(256), 0, s.stream, in, (unsigned long long)n_bytes,
                           (unsigned long long)n_tiles, x4, s.sp_tile.p, s.gsum.p, (unsigned long long)total,
                           (unsigned long long)(tail != n_bytes ? total + 1 : 0), s.doc.buf.p);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(s.doc.buf.p, 0, 8, s.stream));   // no bytes: the single offset 0
    }
    s.doc.commit(docs + 1, true);
    s.doc_gen++;
    *n_docs = docs;
    *tail_start = tail;
    return PFAC_OK;
}

int pfac_slot_doc_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_offsets, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.doc, "pfac_slot_doc_offsets_d2h", "pfac_slot_doc_offsets or pfac_slot_doc_offsets_split", host_offsets, first, n);
}

int pfac_records_segment(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                         pfac_record *d_out, uint64_t out_cap, uint64_t *d_doc_first, uint64_t *n_kept) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_kept) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_kept = 0;
    Slot &s = ctx->slots[slot];
    s.seg_out.invalidate();
    s.seg_first.invalidate();
    const std::string fn = "pfac_records_segment";
    rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE | SCAN_FITS);
    if (rc) return rc;
    const void *src = d_records ? d_records : s.records.p;
    const unsigned long long *off;
    rc = resolve_docs(ctx, s, fn, d_doc_offsets, n_docs, (uintptr_t)d_out | (uintptr_t)d_doc_first, &off);
    if (rc) return rc;
    if (!src && s.last_tiles) return fail(ctx, PFAC_E_ARG, "null record buffer");
    USE_DEVICE(ctx);
    const uint64_t n_tiles = s.last_tiles;
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, n_groups + 1);                 // group prefixes, the total, the offsets' error flag
    if (rc) return rc;
    rc = s.seg_tcnt.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(s.gsum.p + n_groups, 0, 16, s.stream));
    // count (and check the offsets): four groups per 256-thread block, at least one thread per document up to a cap
    const uint64_t gblocks = (n_groups + 3) / 4, vblocks = (n_docs + 255) / 256;
    const unsigned cblocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>(gblocks, std::min<uint64_t>(vblocks, 4096)));
    const int rb = s.last_rec_bytes;
    auto ck = by_width(rb, [](auto w) { return pfac_seg_count_kernel<w()>; });
    hipLaunchKernelGGL(ck, dim3(cblocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)n_tiles,
                       (unsigned long long)s.last_cap, off, (unsigned long long)n_docs, (unsigned long long)s.last_owned,
                       ctx->flen.p, (unsigned)ctx->plan.base.num_final, s.seg_tcnt.p, s.gsum.p, n_groups, s.gsum.p + n_groups + 1);
    if (n_groups) hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
    rc = pass_words(ctx, s, s.gsum.p + n_groups, 2);
    if (rc) return rc;
    const uint64_t total = host_u64(s, H_PASS);
    if (host_u64(s, H_PASS1)) return bad_doc_offsets(ctx, s, fn);
    *n_kept = total;
    if (d_out && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " records kept, out_cap is " + std::to_string(out_cap));
    pfac_record *out;
    unsigned long long *first;
    rc = s.seg_out.bind(ctx, s.stream, d_out, total, total + total / 8 + 4096, &out);
    if (!rc) rc = s.seg_first.bind(ctx, s.stream, d_doc_first, n_docs + 1, docs_cap(n_docs), &first);
    if (rc) return rc;
    if (n_groups) {
        auto wk = by_width(rb, [](auto w) { return pfac_seg_write_kernel<w()>; });
        hipLaunchKernelGGL(wk, dim3((unsigned)gblocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)n_tiles,
                           (unsigned long long)s.last_cap, off, (unsigned long long)n_docs, ctx->flen.p, (unsigned)ctx->plan.base.num_final, s.seg_tcnt.p, s.gsum.p,
                           n_groups, out, first);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(first, 0, (n_docs + 1) * 8, s.stream));   // nothing scanned: every document is empty
    }
    s.seg_out.commit(total, !d_out);
    s.seg_first.commit(n_docs + 1, !d_doc_first);
    s.seg_table = s.last_table;
    return PFAC_OK;
}

int pfac_segment_d2h(pfac_ctx *ctx, int slot, pfac_record *host_records, uint64_t *host_doc_first) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    rc = fetch(ctx, s, s.seg_out, "pfac_segment_d2h", "pfac_records_segment", host_records, 0, s.seg_out.n, true);
    return rc ? rc : fetch(ctx, s, s.seg_first, "pfac_segment_d2h", "pfac_records_segment", host_doc_first, 0, s.seg_first.n, true);
}

int pfac_table_set_state_groups(pfac_ctx *ctx, const uint64_t *masks, uint64_t n_states) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_set_state_groups before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!masks && n_states))
        return fail(ctx, PFAC_E_ARG, "pfac_table_set_state_groups: need num_final masks (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    USE_DEVICE(ctx);
    // as the replacements: a buffer of its own for every call, and freeing the old one waits for the device -- a group
    // pass that still reads the old masks has finished before they go
    ctx->gmask.reset();
    const uint64_t n = std::max<uint64_t>(n_states, 1);
    int rc = ctx->gmask.ensure(ctx, nullptr, n, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(ctx->gmask.p, 0, n * 8));
    if (n_states) HIP_TRY(ctx, hipMemcpy(ctx->gmask.p, masks, n_states * 8, hipMemcpyHostToDevice));
    return PFAC_OK;
}

int pfac_table_set_state_weights(pfac_ctx *ctx, const int32_t *weights, uint64_t n_states) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_set_state_weights before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!weights && n_states))
        return fail(ctx, PFAC_E_ARG, "pfac_table_set_state_weights: need num_final weights (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    USE_DEVICE(ctx);
    // as the state groups: a buffer of its own for every call, and freeing the old one waits for the device
    ctx->sweight.reset();
    const uint64_t n = std::max<uint64_t>(n_states, 1);
    int rc = ctx->sweight.ensure(ctx, nullptr, n, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(ctx->sweight.p, 0, n * 4));
    if (n_states) HIP_TRY(ctx, hipMemcpy(ctx->sweight.p, weights, n_states * 4, hipMemcpyHostToDevice));
    return PFAC_OK;
}

}  // extern "C"

namespace {

// The per-document reductions over the heap (pfac_documents_group_masks: R = GroupOr, `tab` the state groups;
// pfac_documents_scores: R = ScoreAdd, `tab` the state weights; `what` names the table for the error): the checks in
// the header's order, the memset, pfac_doc_reduce_kernel into the slot's buffer `o`, the copy back of the totals and
// the offsets' flag (h_ctl from H_PASS on), and behind the host's check of the flag the copy to the caller's buffer.
template <class R>
int doc_reduce_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const typename R::Tab *tab, const char *what,
                   PassOut<typename R::Out> &o, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                   typename R::Out *d_out) {
    constexpr size_t SZ = sizeof(typename R::Out);
    o.invalidate();
    int rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    if (!tab) return fail(ctx, PFAC_E_STATE, fn + ": no state " + what + " for the uploaded table (pfac_table_set_state_" + what + ")");
    if (!d_doc_offsets && (!s.doc.done || n_docs + 1 != s.doc.n))
        return fail(ctx, PFAC_E_STATE, fn + ": the slot has no document offsets for this n_docs (pfac_slot_doc_offsets, pfac_slot_doc_offsets_split)");
    rc = last_scan_usable(ctx, s, fn, SCAN_FITS);
    if (rc) return rc;
    const unsigned long long *off;
    rc = resolve_docs(ctx, s, fn, d_doc_offsets, n_docs, (uintptr_t)d_out, &off);
    if (rc) return rc;
    if ((uintptr_t)d_out & (SZ - 1)) return fail(ctx, PFAC_E_ARG, fn + ": the output buffer must be aligned to its elements");
    const void *src = d_records ? d_records : (const void *)s.records.p;
    if (s.last_tiles && src != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    USE_DEVICE(ctx);
    const uint64_t n_tiles = n_docs ? s.last_tiles : 0;     // (no documents: the scan owns no bytes, only the offsets are judged)
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, R::RES_WORDS);                 // the totals, the offsets' error flag
    if (rc) return rc;
    // The result is made in the slot's buffer and reaches a caller's only behind the host's check of the offsets' flag:
    // a refused call leaves the caller's buffer as it was.
    typename R::Out *out;
    rc = o.bind(ctx, s.stream, (typename R::Out *)nullptr, std::max<uint64_t>(n_docs, 1), docs_cap(n_docs), &out);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(s.gsum.p, 0, (R::RES_WORDS + 1) * 8, s.stream));
    if (n_docs) HIP_TRY(ctx, hipMemsetAsync(out, 0, n_docs * SZ, s.stream));      // the 0 of every document without a contributing record
    const uint64_t gblocks = (n_groups + 3) / 4, vblocks = (n_docs + 255) / 256;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>(gblocks, std::min<uint64_t>(vblocks, 4096)));
    auto mk = by_width(s.last_rec_bytes, [](auto w) { return pfac_doc_reduce_kernel<w(), R>; });
    hipLaunchKernelGGL(mk, dim3(blocks), dim3(256), 0, s.stream, src, s.tile_index.p, (unsigned long long)n_tiles,
                       (unsigned long long)s.last_cap, off, (unsigned long long)n_docs, (unsigned long long)s.last_owned,
                       ctx->flen.p, tab, (unsigned)ctx->plan.base.num_final, out, n_groups, s.gsum.p);
    rc = pass_words(ctx, s, s.gsum.p, R::RES_WORDS + 1);
    if (rc) return rc;
    if (host_u64(s, H_PASS + 2 * R::RES_WORDS)) return bad_doc_offsets(ctx, s, fn);
    if (d_out && n_docs) HIP_TRY(ctx, hipMemcpyAsync(d_out, out, n_docs * SZ, hipMemcpyDeviceToDevice, s.stream));
    o.commit(n_docs, !d_out);
    return PFAC_OK;
}

}  // namespace

extern "C" {

int pfac_documents_group_masks(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                               uint64_t *d_masks_out, uint64_t *any_mask) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!any_mask) return fail(ctx, PFAC_E_ARG, "null argument");
    *any_mask = 0;
    Slot &s = ctx->slots[slot];
    rc = doc_reduce_run<GroupOr>(ctx, s, "pfac_documents_group_masks", ctx->gmask.p, "groups", s.gm_out, d_records, d_doc_offsets,
                                 n_docs, reinterpret_cast<unsigned long long *>(d_masks_out));
    if (rc == PFAC_OK) *any_mask = host_u64(s, H_PASS);
    return rc;
}

int pfac_documents_scores(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets, uint64_t n_docs,
                          pfac_doc_score *d_scores_out, pfac_doc_score *total) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!total) return fail(ctx, PFAC_E_ARG, "null argument");
    *total = pfac_doc_score{0, 0};
    Slot &s = ctx->slots[slot];
    rc = doc_reduce_run<ScoreAdd>(ctx, s, "pfac_documents_scores", ctx->sweight.p, "weights", s.sc_out, d_records, d_doc_offsets,
                                  n_docs, d_scores_out);
    if (rc == PFAC_OK) *total = pfac_doc_score{(int64_t)host_u64(s, H_PASS), host_u64(s, H_PASS1)};
    return rc;
}

int pfac_selection_document_scores(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first,
                                   uint64_t n_docs, pfac_doc_score *d_scores_out, pfac_doc_score *total) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!total) return fail(ctx, PFAC_E_ARG, "null argument");
    *total = pfac_doc_score{0, 0};
    Slot &s = ctx->slots[slot];
    s.sc_out.invalidate();
    const std::string fn = "pfac_selection_document_scores";
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (!ctx->sweight.p) return fail(ctx, PFAC_E_STATE, fn + ": no state weights for the uploaded table (pfac_table_set_state_weights)");
    const pfac_record *sel = d_sel;
    const unsigned long long *first = reinterpret_cast<const unsigned long long *>(d_doc_first);
    uint64_t n = 0;
    const bool own = !d_sel && !d_doc_first;
    if (own) {                                              // the rules of pfac_selection_count_states' d_sel
        if (!s.scanned || s.pending || !s.ll_out.done || s.ll_seq != s.scan_seq || !s.ll_docs)
            return fail(ctx, PFAC_E_STATE, fn + " needs a pfac_records_leftmost_longest_documents since the slot's last scan");
        if (s.last_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
        rc = s.ll_out.consume(ctx, fn, "selection (d_sel)", d_sel, ANY_N, &sel);
        if (rc) return rc;
        rc = s.lld_first.consume(ctx, fn, "doc_first of the selection (d_doc_first)", d_doc_first, n_docs + 1, &first);
        if (rc) return rc;
        n = s.ll_out.n;
    } else if (!d_sel || !d_doc_first) {
        return fail(ctx, PFAC_E_ARG, fn + ": d_sel and d_doc_first are the slot's (both NULL) or the caller's (neither)");
    }
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if ((((uintptr_t)sel | (uintptr_t)first) & 7) || ((uintptr_t)d_scores_out & 15))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_sel and d_doc_first 8 B, d_scores_out 16 B)");
    USE_DEVICE(ctx);
    if (!own) {                                             // how many records the caller's arrays hold: doc_first[n_docs]
        HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + H_PASS, first + n_docs, 8, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        n = host_u64(s, H_PASS);
    }
    const uint64_t n_waves = (n + SS_RANGE - 1) / SS_RANGE;
    if (n_waves >= (1ull << 33)) return fail(ctx, PFAC_E_ARG, fn + ": too many records");
    rc = ensure_gsum(ctx, s, ScoreAdd::RES_WORDS);
    if (rc) return rc;
    pfac_doc_score *out;
    rc = s.sc_out.bind(ctx, s.stream, (pfac_doc_score *)nullptr, std::max<uint64_t>(n_docs, 1), docs_cap(n_docs), &out);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(s.gsum.p, 0, (ScoreAdd::RES_WORDS + 1) * 8, s.stream));
    if (n_docs) HIP_TRY(ctx, hipMemsetAsync(out, 0, n_docs * sizeof(pfac_doc_score), s.stream));
    const uint64_t vblocks = (n_docs + 255) / 256;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>((n_waves + 3) / 4, std::min<uint64_t>(vblocks, 4096)));
    hipLaunchKernelGGL(pfac_sel_scores_kernel, dim3(blocks), dim3(256), 0, s.stream, sel, (unsigned long long)n, first,
                       (unsigned long long)n_docs, ctx->sweight.p, (unsigned)ctx->plan.base.num_final, out, s.gsum.p);
    rc = pass_words(ctx, s, s.gsum.p, ScoreAdd::RES_WORDS + 1);
    if (rc) return rc;
    if (host_u64(s, H_PASS2))
        return fail(ctx, PFAC_E_ARG, fn + ": d_doc_first must start at 0 and not decrease, and every state of d_sel must be below num_final");
    if (d_scores_out && n_docs)
        HIP_TRY(ctx, hipMemcpyAsync(d_scores_out, out, n_docs * sizeof(pfac_doc_score), hipMemcpyDeviceToDevice, s.stream));
    *total = pfac_doc_score{(int64_t)host_u64(s, H_PASS), host_u64(s, H_PASS1)};
    s.sc_out.commit(n_docs, !d_scores_out);
    return PFAC_OK;
}

int pfac_document_scores_d2h(pfac_ctx *ctx, int slot, pfac_doc_score *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.sc_out, "pfac_document_scores_d2h", "score pass (pfac_documents_scores, pfac_selection_document_scores)", host, first, n);
}

int pfac_group_masks_d2h(pfac_ctx *ctx, int slot, uint64_t *host_masks, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.gm_out, "pfac_group_masks_d2h", "pfac_documents_group_masks", host_masks, first, n);
}

// The offsets' rules alone, on the slot's stream (offsets_rule, for a pass whose first kernel does not carry it): *bad
// becomes non-zero where the offsets do not start at 0, decrease, or do not end at the scan's n_owned.
static void launch_offsets_check(Slot &s, const unsigned long long *off, uint64_t n_docs, unsigned long long *bad) {
    const unsigned vblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 255) / 256, 4096));
    hipLaunchKernelGGL(pfac_offsets_check_kernel, dim3(vblocks), dim3(256), 0, s.stream, off, (unsigned long long)n_docs,
                       (unsigned long long)s.last_owned, bad);
}

// Grid of the output-windowed write kernels (replace, gather) for `total` output bytes: one window of 1 KiB per wave
// while the output is small (every window's search runs in parallel), four above, more where the grid would pass 2^20.
struct WriteGrid {
    unsigned blocks, wins;
};
static WriteGrid write_grid(uint64_t total) {
    uint64_t wins = total >= (64ull << 20) ? 4 : 1;
    const uint64_t max_blocks = 1ull << 20;
    const uint64_t per_block = (uint64_t)RP_WAVES * RP_WIN;
    if ((total + per_block * wins - 1) / (per_block * wins) > max_blocks) wins = (total + per_block * max_blocks - 1) / (per_block * max_blocks);
    return {(unsigned)((total + per_block * wins - 1) / (per_block * wins)), (unsigned)wins};
}

// The three matching calls: the plain one (DM_PLAIN: flags 0 or PFAC_DOCS_INVERT), the one with context lines
// (DM_CONTEXT: flags 0; before / after as the caller gave them) and the one over group masks (DM_GROUPS: d_doc_first
// is the masks, before / after / none_of are all_of / any_of / none_of) and the one over scores (DM_SCORES: d_doc_first
// is the scores, `rule` the windows; with a density `d_doc_offsets` or the slot's offsets are read too: DM_DENSITY).
// One pass: one slot-owned id buffer, one fetch, one lifetime.
static int dm_run(pfac_ctx *ctx, int slot, const std::string &fn, const void *d_doc_first, uint64_t n_docs, int pred,
                  uint64_t before, uint64_t after, uint64_t none_of, uint32_t flags, uint64_t *d_ids_out, uint64_t out_cap,
                  uint64_t *n_matching, const pfac_score_rule *rule = nullptr, const uint64_t *d_doc_offsets = nullptr) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_matching) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_matching = 0;
    Slot &s = ctx->slots[slot];
    s.dm_out.invalidate();
    const bool context = pred == DM_CONTEXT, groups = pred == DM_GROUPS, scores = pred == DM_SCORES;
    const unsigned long long *first, *off = nullptr;
    if (scores) {
        const pfac_doc_score *sc;
        rc = s.sc_out.consume(ctx, fn, "scores of a score pass (n_docs entries)", static_cast<const pfac_doc_score *>(d_doc_first), n_docs, &sc);
        first = reinterpret_cast<const unsigned long long *>(sc);
        if (rc == PFAC_OK && !rule) rc = fail(ctx, PFAC_E_ARG, fn + ": null rule");
        if (rc == PFAC_OK && rule->density_den) {
            off = reinterpret_cast<const unsigned long long *>(d_doc_offsets);
            if (!off && !s.doc.done) rc = fail(ctx, PFAC_E_STATE, fn + ": no document offsets for the slot (pfac_slot_doc_offsets)");
            else if (!off && n_docs + 1 != s.doc.n) rc = fail(ctx, PFAC_E_ARG, fn + ": n_docs differs from the slot's document offsets");
            else if (!off) off = s.doc.buf.p;
        }
        if (rc == PFAC_OK && ((((uintptr_t)first) & 15) || ((uintptr_t)off & 7)))
            rc = fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_scores 16 B, d_doc_offsets 8 B)");
    } else {
        const uint64_t *df = static_cast<const uint64_t *>(d_doc_first);
        rc = groups ? s.gm_out.consume(ctx, fn, "group masks of a pfac_documents_group_masks (n_docs entries)", df, n_docs, &first)
                    : s.seg_first.consume(ctx, fn, "doc_first of a pfac_records_segment (n_docs + 1 entries)", df, n_docs + 1, &first);
    }
    if (rc) return rc;
    if (context && flags) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 (context around non-matching documents is not defined by doc_first)");
    if (flags > PFAC_DOCS_INVERT) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 or PFAC_DOCS_INVERT");
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if (((uintptr_t)first | (uintptr_t)d_ids_out) & 7) return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    USE_DEVICE(ctx);
    const unsigned n_groups = (unsigned)((n_docs + DM_BLOCKS * WAVE - 1) / (DM_BLOCKS * WAVE));
    // (a window wider than the input is the input; the groups form passes its sets as they are)
    const unsigned long long bef = groups ? before : std::min(before, n_docs), aft = groups ? after : std::min(after, n_docs);
    const dim3 grid((n_groups + 3) / 4), block(256);
    const pfac_doc_score *sc = reinterpret_cast<const pfac_doc_score *>(first);
    uint64_t total = 0;
    if (n_groups) {
        rc = ensure_gsum(ctx, s, n_groups);
        if (rc) return rc;
        if (scores && off)
            hipLaunchKernelGGL((pfac_docs_scores_kernel<false, true>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, (unsigned)flags,
                               *rule, off, s.gsum.p, n_groups, 0ull, (unsigned long long *)nullptr);
        else if (scores)
            hipLaunchKernelGGL((pfac_docs_scores_kernel<false, false>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, (unsigned)flags,
                               *rule, off, s.gsum.p, n_groups, 0ull, (unsigned long long *)nullptr);
        else if (groups)
            hipLaunchKernelGGL(pfac_docs_groups_kernel<false>, grid, block, 0, s.stream, first, (unsigned long long)n_docs, (unsigned)flags,
                               bef, aft, (unsigned long long)none_of, s.gsum.p, n_groups, 0ull, (unsigned long long *)nullptr);
        else if (context)
            hipLaunchKernelGGL(pfac_docs_context_kernel<false>, grid, block, 0, s.stream, first, (unsigned long long)n_docs, bef, aft,
                               s.gsum.p, n_groups, 0ull, (unsigned long long *)nullptr);
        else
            hipLaunchKernelGGL(pfac_docs_matching_kernel<false>, grid, block, 0, s.stream, first,
                               (unsigned long long)n_docs, (unsigned)flags, s.gsum.p, n_groups, 0ull, (unsigned long long *)nullptr);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
        rc = pass_words(ctx, s, s.gsum.p + n_groups, 1);
        if (rc) return rc;
        total = host_u64(s, H_PASS);
    }
    *n_matching = total;
    if (d_ids_out && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " documents, out_cap is " + std::to_string(out_cap));
    unsigned long long *ids;
    rc = s.dm_out.bind(ctx, s.stream, d_ids_out, total, total + total / 8 + 4096, &ids);
    if (rc) return rc;
    if (total) {
        if (scores && off)
            hipLaunchKernelGGL((pfac_docs_scores_kernel<true, true>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, (unsigned)flags,
                               *rule, off, s.gsum.p, n_groups, (unsigned long long)total, ids);
        else if (scores)
            hipLaunchKernelGGL((pfac_docs_scores_kernel<true, false>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, (unsigned)flags,
                               *rule, off, s.gsum.p, n_groups, (unsigned long long)total, ids);
        else if (groups)
            hipLaunchKernelGGL(pfac_docs_groups_kernel<true>, grid, block, 0, s.stream, first, (unsigned long long)n_docs, (unsigned)flags,
                               bef, aft, (unsigned long long)none_of, s.gsum.p, n_groups, (unsigned long long)total, ids);
        else if (context)
            hipLaunchKernelGGL(pfac_docs_context_kernel<true>, grid, block, 0, s.stream, first, (unsigned long long)n_docs, bef, aft,
                               s.gsum.p, n_groups, (unsigned long long)total, ids);
        else
            hipLaunchKernelGGL(pfac_docs_matching_kernel<true>, grid, block, 0, s.stream, first,
                               (unsigned long long)n_docs, (unsigned)flags, s.gsum.p, n_groups, (unsigned long long)total, ids);
        HIP_TRY(ctx, hipGetLastError());
    }
    s.dm_out.commit(total, !d_ids_out);
    return PFAC_OK;
}

int pfac_documents_matching(pfac_ctx *ctx, int slot, const uint64_t *d_doc_first, uint64_t n_docs, uint32_t flags,
                            uint64_t *d_ids_out, uint64_t out_cap, uint64_t *n_matching) {
    return dm_run(ctx, slot, "pfac_documents_matching", d_doc_first, n_docs, DM_PLAIN, 0, 0, 0, flags, d_ids_out, out_cap, n_matching);
}

int pfac_documents_matching_context(pfac_ctx *ctx, int slot, const uint64_t *d_doc_first, uint64_t n_docs, uint64_t before,
                                    uint64_t after, uint32_t flags, uint64_t *d_ids_out, uint64_t out_cap, uint64_t *n_matching) {
    return dm_run(ctx, slot, "pfac_documents_matching_context", d_doc_first, n_docs, DM_CONTEXT, before, after, 0, flags, d_ids_out,
                  out_cap, n_matching);
}

int pfac_documents_matching_groups(pfac_ctx *ctx, int slot, const uint64_t *d_masks, uint64_t n_docs, uint64_t all_of,
                                   uint64_t any_of, uint64_t none_of, uint32_t flags, uint64_t *d_ids_out, uint64_t out_cap,
                                   uint64_t *n_matching) {
    return dm_run(ctx, slot, "pfac_documents_matching_groups", d_masks, n_docs, DM_GROUPS, all_of, any_of, none_of, flags, d_ids_out,
                  out_cap, n_matching);
}

int pfac_documents_matching_scores(pfac_ctx *ctx, int slot, const pfac_doc_score *d_scores, const uint64_t *d_doc_offsets,
                                   uint64_t n_docs, const pfac_score_rule *rule, uint32_t flags, uint64_t *d_ids_out,
                                   uint64_t out_cap, uint64_t *n_matching) {
    return dm_run(ctx, slot, "pfac_documents_matching_scores", d_scores, n_docs, DM_SCORES, 0, 0, 0, flags, d_ids_out, out_cap,
                  n_matching, rule, d_doc_offsets);
}

int pfac_documents_matching_d2h(pfac_ctx *ctx, int slot, uint64_t *host_ids) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.dm_out, "pfac_documents_matching_d2h", "pfac_documents_matching", host_ids, 0, s.dm_out.n);
}

// The k best documents: the select (its passes and picks queued back to back, then the ONE copy back: n_top), the
// compaction, and under PFAC_TOP_RANKED the sort.  The ids are dm_out's -- one pass with the matching calls.
int pfac_documents_top_scores(pfac_ctx *ctx, int slot, const pfac_doc_score *d_scores, const uint64_t *d_doc_offsets,
                              uint64_t n_docs, const pfac_score_rule *rule, uint32_t rule_flags, uint64_t k, uint32_t flags,
                              uint64_t *d_ids_out, uint64_t out_cap, pfac_doc_score *d_top_scores_out, uint64_t *n_top) {
    const std::string fn = "pfac_documents_top_scores";
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_top) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_top = 0;
    Slot &s = ctx->slots[slot];
    s.dm_out.invalidate();
    s.tp_out.invalidate();
    const pfac_doc_score *sc;
    const unsigned long long *off = nullptr;
    rc = s.sc_out.consume(ctx, fn, "scores of a score pass (n_docs entries)", d_scores, n_docs, &sc);
    if (rc == PFAC_OK && rule && rule->density_den) {
        off = reinterpret_cast<const unsigned long long *>(d_doc_offsets);
        if (!off && !s.doc.done) rc = fail(ctx, PFAC_E_STATE, fn + ": no document offsets for the slot (pfac_slot_doc_offsets)");
        else if (!off && n_docs + 1 != s.doc.n) rc = fail(ctx, PFAC_E_ARG, fn + ": n_docs differs from the slot's document offsets");
        else if (!off) off = s.doc.buf.p;
    }
    if (rc == PFAC_OK && (((uintptr_t)sc & 15) || ((uintptr_t)off & 7)))
        rc = fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_scores 16 B, d_doc_offsets 8 B)");
    if (rc) return rc;
    if (rule_flags > PFAC_DOCS_INVERT) return fail(ctx, PFAC_E_ARG, fn + ": rule_flags must be 0 or PFAC_DOCS_INVERT");
    if (flags & ~(PFAC_TOP_BY_COUNT | PFAC_TOP_LOWEST | PFAC_TOP_RANKED))
        return fail(ctx, PFAC_E_ARG, fn + ": flags outside PFAC_TOP_BY_COUNT | PFAC_TOP_LOWEST | PFAC_TOP_RANKED");
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if (((uintptr_t)d_ids_out & 7) || ((uintptr_t)d_top_scores_out & 15))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_ids_out 8 B, d_top_scores_out 16 B)");
    USE_DEVICE(ctx);
    // no rule: every document is a candidate
    const pfac_score_rule r = rule ? *rule : pfac_score_rule{INT64_MIN, INT64_MAX, 0, UINT64_MAX, 0, 0};
    const unsigned invert = rule ? (unsigned)rule_flags : 0u;
    uint64_t total = 0;
    if (n_docs && k) {
        rc = s.tp_work.ensure(ctx, s.stream, TOP_WORK_WORDS, TOP_WORK_WORDS);
        if (rc) return rc;
        unsigned long long *work = s.tp_work.p;
        HIP_TRY(ctx, hipMemsetAsync(work, 0, TOP_WORK_WORDS * sizeof(unsigned long long), s.stream));
        const dim3 hgrid((unsigned)std::min<uint64_t>((n_docs + TOP_BINS - 1) / TOP_BINS, 2048)), hblock(TOP_BINS);
        for (int pass = 0; pass < TOP_PASSES; pass++) {
            if (off)
                hipLaunchKernelGGL(pfac_top_hist_kernel<true>, hgrid, hblock, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                                   (unsigned)flags, pass, (unsigned long long)k, work);
            else
                hipLaunchKernelGGL(pfac_top_hist_kernel<false>, hgrid, hblock, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                                   (unsigned)flags, pass, (unsigned long long)k, work);
        }
        hipLaunchKernelGGL(pfac_top_final_kernel, dim3(1), dim3(WAVE), 0, s.stream, work, (unsigned long long)k);
        rc = pass_words(ctx, s, work + TOP_NCAND, 1);           // (written by the second pass: the first histograms' sum)
        if (rc) return rc;
        total = std::min<uint64_t>(k, host_u64(s, H_PASS));
    }
    *n_top = total;
    if ((d_ids_out || d_top_scores_out) && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " documents, out_cap is " + std::to_string(out_cap));
    unsigned long long *ids;
    pfac_doc_score *top;
    rc = s.dm_out.bind(ctx, s.stream, d_ids_out, total, total + total / 8 + 4096, &ids);
    if (rc) return rc;
    rc = s.tp_out.bind(ctx, s.stream, d_top_scores_out, total, total + total / 8 + 4096, &top);
    if (rc) return rc;
    if (total) {
        const bool ranked = (flags & PFAC_TOP_RANKED) != 0;
        const unsigned n_groups = (unsigned)((n_docs + DM_BLOCKS * WAVE - 1) / (DM_BLOCKS * WAVE));
        const unsigned n_blocks = (unsigned)((total + TS_BLOCK - 1) / TS_BLOCK);
        rc = ensure_gsum(ctx, s, 2 * n_groups + 1);          // the group prefixes of the keys in front of T and their total, the same of the keys equal to T
        if (rc) return rc;
        if (ranked) {
            rc = s.tp_ent.ensure(ctx, s.stream, 2 * total, 2 * (total + total / 8 + 4096));
            if (rc) return rc;
        }
        if (ranked && total > TS_BLOCK) {
            rc = s.tp_bh.ensure(ctx, s.stream, (uint64_t)TOP_BINS * n_blocks + 1, (uint64_t)TOP_BINS * quarter_more(n_blocks) + 1);
            if (rc) return rc;
        }
        const unsigned long long *st = s.tp_work.p;
        const bool one = total <= TS_BLOCK;                      // the sort in one workgroup
        unsigned long long *bsum = s.gsum.p, *esum = s.gsum.p + n_groups + 1;
        ulonglong2 *ent = ranked ? s.tp_ent.p : nullptr;
        const dim3 grid((n_groups + 3) / 4), block(256);
        if (off) {
            hipLaunchKernelGGL((pfac_top_compact_kernel<false, true>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                               (unsigned)flags, st, bsum, esum, n_groups, 0ull, (unsigned long long *)nullptr, (pfac_doc_score *)nullptr, (ulonglong2 *)nullptr);
        } else {
            hipLaunchKernelGGL((pfac_top_compact_kernel<false, false>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                               (unsigned)flags, st, bsum, esum, n_groups, 0ull, (unsigned long long *)nullptr, (pfac_doc_score *)nullptr, (ulonglong2 *)nullptr);
        }
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, bsum, n_groups);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, esum, n_groups);
        if (off) {
            hipLaunchKernelGGL((pfac_top_compact_kernel<true, true>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                               (unsigned)flags, st, bsum, esum, n_groups, (unsigned long long)total, ids, top, ent);
        } else {
            hipLaunchKernelGGL((pfac_top_compact_kernel<true, false>), grid, block, 0, s.stream, sc, (unsigned long long)n_docs, invert, r, off,
                               (unsigned)flags, st, bsum, esum, n_groups, (unsigned long long)total, ids, top, ent);
        }
        if (ranked && one) {
            hipLaunchKernelGGL(pfac_top_sort_one_kernel, dim3(1), dim3(TS_WAVES * WAVE), 0, s.stream, (const ulonglong2 *)ent,
                               (unsigned long long)total, ids, top, sc, (unsigned long long)n_docs);
        } else if (ranked) {
            ulonglong2 *a = ent, *b = ent + total;
            for (int pass = 0; pass < TOP_PASSES; pass++) {
                const bool last = pass == TOP_PASSES - 1;
                hipLaunchKernelGGL(pfac_top_sort_hist_kernel, dim3(n_blocks), dim3(TS_WAVES * WAVE), 0, s.stream, (const ulonglong2 *)a,
                                   (unsigned long long)total, pass * TOP_BITS, n_blocks, s.tp_bh.p);
                hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.tp_bh.p, (unsigned)TOP_BINS * n_blocks);
                hipLaunchKernelGGL(pfac_top_sort_scatter_kernel, dim3(n_blocks), dim3(TS_WAVES * WAVE), 0, s.stream, (const ulonglong2 *)a,
                                   (unsigned long long)total, pass * TOP_BITS, n_blocks, (const unsigned long long *)s.tp_bh.p,
                                   last ? (ulonglong2 *)nullptr : b, ids, top, sc, (unsigned long long)n_docs);
                std::swap(a, b);
            }
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    s.dm_out.commit(total, !d_ids_out);
    s.tp_out.commit(total, !d_top_scores_out);
    return PFAC_OK;
}

int pfac_documents_top_scores_d2h(pfac_ctx *ctx, int slot, pfac_doc_score *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.tp_out, "pfac_documents_top_scores_d2h", "pfac_documents_top_scores", host, first, n);
}

// Term counts: the key kernel (with the checks), the sort, the heads and their group prefix queued back to back, then the
// ONE copy back (the total and the error word); behind the host's checks the write, the counts and row_ptr.
int pfac_documents_term_counts(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first, uint64_t n_docs,
                               uint32_t flags, uint64_t *d_row_ptr_out, uint32_t *d_states_out, uint32_t *d_counts_out,
                               uint64_t out_cap, uint64_t *n_terms) {
    const std::string fn = "pfac_documents_term_counts";
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_terms) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_terms = 0;
    Slot &s = ctx->slots[slot];
    s.tc_row.invalidate();
    s.tc_st.invalidate();
    s.tc_cnt.invalidate();
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    const pfac_record *sel = d_sel;
    const unsigned long long *first = reinterpret_cast<const unsigned long long *>(d_doc_first);
    uint64_t n = 0;
    const bool own = !d_sel && !d_doc_first;
    if (own && flags == PFAC_TERMS_SELECTION) {             // the rules of pfac_selection_count_states' d_sel
        if (!s.scanned || s.pending || !s.ll_out.done || s.ll_seq != s.scan_seq || !s.ll_docs)
            return fail(ctx, PFAC_E_STATE, fn + " needs a pfac_records_leftmost_longest_documents since the slot's last scan");
        if (s.last_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
        if (!s.ll_out.own || !s.lld_first.done || !s.lld_first.own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no selection (it went to the caller's buffers; pass those)");
    } else if (own && flags == 0) {
        if (!s.seg_out.done || !s.seg_out.own || !s.seg_first.done || !s.seg_first.own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no pfac_records_segment result (none yet, or it went to the caller's buffers; pass those)");
        if (s.seg_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the segment pass ran with an earlier table");
    }
    if (flags > PFAC_TERMS_SELECTION) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 or PFAC_TERMS_SELECTION");
    if (own) {
        const bool picks = flags == PFAC_TERMS_SELECTION;
        rc = (picks ? s.ll_out : s.seg_out).consume(ctx, fn, "records (d_sel)", d_sel, ANY_N, &sel);
        if (rc) return rc;
        rc = (picks ? s.lld_first : s.seg_first).consume(ctx, fn, "doc_first (d_doc_first)", d_doc_first, n_docs + 1, &first);
        if (rc) return rc;
        n = picks ? s.ll_out.n : s.seg_out.n;
    } else if (!d_sel || !d_doc_first) {
        return fail(ctx, PFAC_E_ARG, fn + ": d_sel and d_doc_first are the slot's (both NULL) or the caller's (neither)");
    }
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if ((((uintptr_t)sel | (uintptr_t)first | (uintptr_t)d_row_ptr_out) & 7) || (((uintptr_t)d_states_out | (uintptr_t)d_counts_out) & 3))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_sel, d_doc_first and d_row_ptr_out 8 B, d_states_out and d_counts_out 4 B)");
    USE_DEVICE(ctx);
    if (!own) {                                             // how many records the caller's arrays hold: doc_first[n_docs]
        HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + H_PASS, first + n_docs, 8, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        n = host_u64(s, H_PASS);
    }
    if (n >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": the record count, d_doc_first[n_docs], must be below 2^32");
    const char *rules = ": d_doc_first must start at 0 and not decrease, and every state of d_sel must be below num_final";
    if (n_docs == 0 && n) return fail(ctx, PFAC_E_ARG, fn + rules);
    const unsigned num_final = (unsigned)ctx->plan.base.num_final;
    auto bit_width = [](uint64_t v) { unsigned b = 0; while (v) { b++; v >>= 1; } return b; };
    const unsigned sbits = bit_width(num_final ? num_final - 1 : 0), dbits = bit_width(n_docs ? n_docs - 1 : 0);
    const int passes = (int)((sbits + dbits + TOP_BITS - 1) / TOP_BITS);
    const unsigned n_groups = (unsigned)((n + DM_BLOCKS * WAVE - 1) / (DM_BLOCKS * WAVE));
    const uint64_t n_heads_blocks = (n + WAVE - 1) / WAVE;
    rc = ensure_gsum(ctx, s, n_groups + 1);                 // the group prefixes, the total, the error word
    if (rc) return rc;
    unsigned long long *res = s.gsum.p + n_groups;
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
    const unsigned long long *sorted = nullptr;
    if (n) {
        rc = s.tc_keys.ensure(ctx, s.stream, 2 * n, 2 * (n + n / 8 + 4096));
        if (!rc) rc = s.tc_bal.ensure(ctx, s.stream, n_heads_blocks, quarter_more(n_heads_blocks));
        if (!rc) rc = s.tc_x.ensure(ctx, s.stream, n_heads_blocks, quarter_more(n_heads_blocks));
        if (!rc) rc = tc_sort_reserve(ctx, s, n, passes);
        if (rc) return rc;
    }
    if (n_docs) {
        const uint64_t n_waves = (n + SS_RANGE - 1) / SS_RANGE, vblocks = (n_docs + 255) / 256;
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>((n_waves + 3) / 4, std::min<uint64_t>(vblocks, 4096)));
        hipLaunchKernelGGL(pfac_tc_key_kernel, dim3(blocks), dim3(256), 0, s.stream, sel, (unsigned long long)n, first,
                           (unsigned long long)n_docs, num_final, sbits, s.tc_keys.p, res + 1);
    }
    if (n) {
        sorted = tc_sort(ctx, s, n, passes);
        hipLaunchKernelGGL(pfac_tc_heads_kernel, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, sorted, (unsigned long long)n,
                           s.tc_bal.p, s.tc_x.p, s.gsum.p, n_groups);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
    }
    rc = pass_words(ctx, s, res, 2);
    if (rc) return rc;
    if (host_u64(s, H_PASS1)) return fail(ctx, PFAC_E_ARG, fn + rules);
    const uint64_t total = host_u64(s, H_PASS);
    *n_terms = total;
    if ((d_states_out || d_counts_out) && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " terms, out_cap is " + std::to_string(out_cap));
    unsigned long long *row;
    unsigned *st, *cn;
    rc = s.tc_row.bind(ctx, s.stream, d_row_ptr_out, n_docs + 1, docs_cap(n_docs), &row);
    if (!rc) rc = s.tc_st.bind(ctx, s.stream, d_states_out, total, total + total / 8 + 4096, &st);
    if (!rc) rc = s.tc_cnt.bind(ctx, s.stream, d_counts_out, total, total + total / 8 + 4096, &cn);
    if (!rc) rc = s.tc_hidx.ensure(ctx, s.stream, total + 1, total + total / 8 + 4096);
    if (rc) return rc;
    if (total) {
        hipLaunchKernelGGL(pfac_tc_write_kernel, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, sorted, (unsigned long long)n,
                           (const unsigned long long *)s.tc_bal.p, (const unsigned *)s.tc_x.p, (const unsigned long long *)s.gsum.p, n_groups,
                           (1ull << sbits) - 1ull, (unsigned long long)total, st, s.tc_hidx.p);
        const unsigned cblocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(pfac_tc_counts_kernel, dim3(cblocks), dim3(256), 0, s.stream, (const unsigned *)s.tc_hidx.p,
                           (unsigned long long)total, cn);
        const unsigned rblocks = (unsigned)std::min<uint64_t>((n_docs + 1 + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(pfac_tc_rowptr_kernel, dim3(rblocks), dim3(256), 0, s.stream, first, (unsigned long long)n_docs,
                           (unsigned long long)n, (const unsigned long long *)s.tc_bal.p, (const unsigned *)s.tc_x.p,
                           (const unsigned long long *)s.gsum.p, (unsigned long long)total, row);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(row, 0, (n_docs + 1) * 8, s.stream));     // no record: every document is empty
    }
    s.tc_table = ctx->table_gen;
    s.tc_row.commit(n_docs + 1, !d_row_ptr_out);
    s.tc_st.commit(total, !d_states_out);
    s.tc_cnt.commit(total, !d_counts_out);
    return PFAC_OK;
}

int pfac_documents_term_counts_d2h(pfac_ctx *ctx, int slot, uint64_t *host_row_ptr, uint32_t *host_states, uint32_t *host_counts) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const char *me = "pfac_documents_term_counts_d2h", *pass = "pfac_documents_term_counts";
    rc = fetch(ctx, s, s.tc_row, me, pass, host_row_ptr, 0, s.tc_row.n, true);
    if (!rc) rc = fetch(ctx, s, s.tc_st, me, pass, host_states, 0, s.tc_st.n, true);
    return rc ? rc : fetch(ctx, s, s.tc_cnt, me, pass, host_counts, 0, s.tc_cnt.n, true);
}

// The rule table: validated whole on the host (a refused call keeps the earlier rules), inverted to state-major by a
// counting sort -- the rules ascend inside a state because they are visited in order -- and uploaded as the state groups
// are: buffers of their own for every call, and freeing the old ones waits for the device.
int pfac_table_set_rules(pfac_ctx *ctx, const uint64_t *rule_ptr, const uint32_t *terms, const uint32_t *need, uint64_t n_rules) {
    const std::string fn = "pfac_table_set_rules";
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    const uint64_t num_final = (uint64_t)ctx->plan.base.num_final;
    std::vector<unsigned> sptr(num_final + 1, 0u), ent;
    if (n_rules) {
        if (!rule_ptr || !need) return fail(ctx, PFAC_E_ARG, fn + ": null rule_ptr or need");
        if (n_rules >= (1ull << 31)) return fail(ctx, PFAC_E_ARG, fn + ": n_rules must be below 2^31");
        if (rule_ptr[0] != 0) return fail(ctx, PFAC_E_ARG, fn + ": rule_ptr[0] must be 0");
        for (uint64_t r = 0; r < n_rules; r++)
            if (rule_ptr[r + 1] < rule_ptr[r]) return fail(ctx, PFAC_E_ARG, fn + ": rule_ptr decreases at rule " + std::to_string(r));
        const uint64_t n_terms = rule_ptr[n_rules];
        if (n_terms >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": the rules must hold fewer than 2^32 terms");
        if (n_terms && !terms) return fail(ctx, PFAC_E_ARG, fn + ": null terms");
        std::vector<unsigned> seen(num_final, 0u);              // the last rule (+ 1) that named the state
        for (uint64_t r = 0; r < n_rules; r++) {
            uint64_t positive = 0;
            for (uint64_t t = rule_ptr[r]; t < rule_ptr[r + 1]; t++) {
                const uint32_t st = terms[t] & ~PFAC_RULE_NOT;
                if (st >= num_final)
                    return fail(ctx, PFAC_E_ARG, fn + ": rule " + std::to_string(r) + " names state " + std::to_string(st) + ", num_final is " + std::to_string(num_final));
                if (seen[st] == (unsigned)r + 1u)
                    return fail(ctx, PFAC_E_ARG, fn + ": rule " + std::to_string(r) + " names state " + std::to_string(st) + " twice");
                seen[st] = (unsigned)r + 1u;
                positive += !(terms[t] & PFAC_RULE_NOT);
                sptr[st + 1]++;
            }
            if (need[r] == 0 || need[r] > positive)
                return fail(ctx, PFAC_E_ARG, fn + ": need of rule " + std::to_string(r) + " is " + std::to_string(need[r]) + ", it has " + std::to_string(positive) + " positive terms");
        }
        for (uint64_t st = 0; st < num_final; st++) sptr[st + 1] += sptr[st];
        ent.resize(n_terms);
        std::vector<unsigned> at(sptr.begin(), sptr.end() - 1);
        for (uint64_t r = 0; r < n_rules; r++)
            for (uint64_t t = rule_ptr[r]; t < rule_ptr[r + 1]; t++)
                ent[at[terms[t] & ~PFAC_RULE_NOT]++] = (unsigned)r << 1 | (terms[t] >> 31);
    }
    USE_DEVICE(ctx);
    ctx->ru_sptr.reset(); ctx->ru_ent.reset(); ctx->ru_need.reset();
    ctx->ru_n = ctx->ru_terms = 0;
    if (!n_rules) return PFAC_OK;
    const uint64_t n_ent = std::max<uint64_t>(ent.size(), 1);
    int rc = ctx->ru_sptr.ensure(ctx, nullptr, num_final + 1, num_final + 1);
    if (!rc) rc = ctx->ru_ent.ensure(ctx, nullptr, n_ent, n_ent);
    if (!rc) rc = ctx->ru_need.ensure(ctx, nullptr, n_rules, n_rules);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->ru_sptr.p, sptr.data(), (num_final + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(ctx->ru_ent.p, 0, n_ent * 4));
    if (!ent.empty()) HIP_TRY(ctx, hipMemcpy(ctx->ru_ent.p, ent.data(), ent.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->ru_need.p, need, n_rules * 4, hipMemcpyHostToDevice));
    ctx->ru_n = n_rules;
    ctx->ru_terms = ent.size();
    return PFAC_OK;
}

// Rule sets: the count kernel (with the checks) and its group prefix, then the FIRST copy back (E and the error word:
// E sizes the expand); the expand, the sort, the fired tails and their group prefix, then the second (the total); behind
// the host's overflow check the write and row_ptr.
int pfac_documents_rules(pfac_ctx *ctx, int slot, const uint64_t *d_row_ptr, const uint32_t *d_states, uint64_t n_docs, uint32_t flags,
                         uint64_t *d_row_ptr_out, uint32_t *d_rules_out, uint64_t out_cap, uint64_t *n_fired) {
    const std::string fn = "pfac_documents_rules";
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_fired) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_fired = 0;
    Slot &s = ctx->slots[slot];
    s.ru_row.invalidate();
    s.ru_out.invalidate();
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (!ctx->ru_n) return fail(ctx, PFAC_E_STATE, fn + ": no rules for the uploaded table (pfac_table_set_rules)");
    const unsigned long long *row_in = reinterpret_cast<const unsigned long long *>(d_row_ptr);
    const unsigned *st_in = d_states;
    const bool own = !d_row_ptr && !d_states;
    uint64_t n = 0;
    if (own) {
        if (!s.tc_row.done || !s.tc_row.own || !s.tc_st.done || !s.tc_st.own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no pfac_documents_term_counts result (none yet, or it went to the caller's buffers; pass those)");
        if (s.tc_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the term counts were made with an earlier table");
    } else if (!d_row_ptr || !d_states) {
        return fail(ctx, PFAC_E_ARG, fn + ": d_row_ptr and d_states are the slot's (both NULL) or the caller's (neither)");
    }
    if (flags) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0");
    if (own) {
        rc = s.tc_row.consume(ctx, fn, "row_ptr (d_row_ptr)", d_row_ptr, n_docs + 1, &row_in);
        if (!rc) rc = s.tc_st.consume(ctx, fn, "states (d_states)", d_states, ANY_N, &st_in);
        if (rc) return rc;
        n = s.tc_st.n;
    }
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if ((((uintptr_t)row_in | (uintptr_t)d_row_ptr_out) & 7) || (((uintptr_t)st_in | (uintptr_t)d_rules_out) & 3))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_row_ptr and d_row_ptr_out 8 B, d_states and d_rules_out 4 B)");
    USE_DEVICE(ctx);
    if (!own) {                                             // how many pairs the caller's arrays hold: row_ptr[n_docs]
        HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + H_PASS, row_in + n_docs, 8, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        n = host_u64(s, H_PASS);
    }
    if (n >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": the pair count, d_row_ptr[n_docs], must be below 2^32");
    const char *broken = ": d_row_ptr must start at 0 and not decrease, and the states of a row must strictly ascend below num_final";
    if (n_docs == 0 && n) return fail(ctx, PFAC_E_ARG, fn + broken);
    const unsigned num_final = (unsigned)ctx->plan.base.num_final;
    auto bit_width = [](uint64_t v) { unsigned b = 0; while (v) { b++; v >>= 1; } return b; };
    const unsigned rbits = bit_width(ctx->ru_n - 1), dbits = bit_width(n_docs ? n_docs - 1 : 0);
    const unsigned rmask = (unsigned)((1ull << rbits) - 1ull);
    const int passes = (int)((dbits + rbits + 1 + TOP_BITS - 1) / TOP_BITS);
    // 1. the keys of every pair
    const unsigned p_groups = (unsigned)((n + DM_BLOCKS * WAVE - 1) / (DM_BLOCKS * WAVE));
    rc = s.ru_gsum.ensure(ctx, s.stream, (uint64_t)p_groups + 2, quarter_more(p_groups) + 2);
    if (!rc && n) rc = s.ru_cpre.ensure(ctx, s.stream, n, n + n / 8 + 4096);
    if (!rc && n) rc = s.ru_doc.ensure(ctx, s.stream, n, n + n / 8 + 4096);
    if (rc) return rc;
    unsigned long long *pres = s.ru_gsum.p + p_groups;
    HIP_TRY(ctx, hipMemsetAsync(pres, 0, 16, s.stream));
    if (n_docs) {
        const uint64_t vblocks = (n_docs + 255) / 256;
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>(((uint64_t)p_groups + 3) / 4, std::min<uint64_t>(vblocks, 4096)));
        hipLaunchKernelGGL(pfac_ru_count_kernel, dim3(blocks), dim3(256), 0, s.stream, row_in, (unsigned long long)n_docs, st_in,
                           (unsigned long long)n, (const unsigned *)ctx->ru_sptr.p, num_final, s.ru_cpre.p, s.ru_doc.p, s.ru_gsum.p,
                           p_groups, pres + 1);
        if (p_groups) hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.ru_gsum.p, p_groups);
    }
    rc = pass_words(ctx, s, pres, 2);
    if (rc) return rc;
    if (host_u64(s, H_PASS1)) return fail(ctx, PFAC_E_ARG, fn + broken);
    const uint64_t E = host_u64(s, H_PASS);
    if (E >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": the pairs expand into " + std::to_string(E) + " (document, rule) entries, the limit is 2^32 - 1");
    // 2. - 4. expand, sort, the fired tails
    const unsigned n_groups = (unsigned)((E + DM_BLOCKS * WAVE - 1) / (DM_BLOCKS * WAVE));
    const uint64_t n_blocks64 = (E + WAVE - 1) / WAVE;
    const unsigned long long *sorted = nullptr;
    uint64_t total = 0;
    if (E) {
        rc = ensure_gsum(ctx, s, n_groups);
        if (!rc) rc = s.tc_keys.ensure(ctx, s.stream, 2 * E, 2 * (E + E / 8 + 4096));
        if (!rc) rc = s.tc_bal.ensure(ctx, s.stream, n_blocks64, quarter_more(n_blocks64));
        if (!rc) rc = s.tc_x.ensure(ctx, s.stream, n_blocks64, quarter_more(n_blocks64));
        if (!rc) rc = tc_sort_reserve(ctx, s, E, passes);
        if (rc) return rc;
        const unsigned eblocks = (unsigned)std::min<uint64_t>((E + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(pfac_ru_expand_kernel, dim3(eblocks), dim3(256), 0, s.stream, st_in, (unsigned long long)n,
                           (const unsigned *)s.ru_cpre.p, (const unsigned *)s.ru_doc.p, (const unsigned long long *)s.ru_gsum.p, p_groups,
                           (const unsigned *)ctx->ru_sptr.p, (const unsigned *)ctx->ru_ent.p, rbits, (unsigned long long)E, s.tc_keys.p);
        sorted = tc_sort(ctx, s, E, passes);
        hipLaunchKernelGGL(pfac_ru_fired_kernel, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, sorted, (unsigned long long)E,
                           (const unsigned *)ctx->ru_need.p, rmask, s.tc_bal.p, s.tc_x.p, s.gsum.p, n_groups);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
        rc = pass_words(ctx, s, s.gsum.p + n_groups, 1);
        if (rc) return rc;
        total = host_u64(s, H_PASS);
    }
    *n_fired = total;
    if (d_rules_out && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " fired rules, out_cap is " + std::to_string(out_cap));
    // 5. the write and row_ptr
    unsigned long long *row;
    unsigned *out;
    rc = s.ru_row.bind(ctx, s.stream, d_row_ptr_out, n_docs + 1, docs_cap(n_docs), &row);
    if (!rc) rc = s.ru_out.bind(ctx, s.stream, d_rules_out, total, total + total / 8 + 4096, &out);
    if (rc) return rc;
    if (total) {
        hipLaunchKernelGGL(pfac_ru_write_kernel, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, sorted, (unsigned long long)E,
                           (const unsigned long long *)s.tc_bal.p, (const unsigned *)s.tc_x.p, (const unsigned long long *)s.gsum.p, n_groups,
                           rmask, (unsigned long long)total, out);
        const unsigned rblocks = (unsigned)std::min<uint64_t>((n_docs + 1 + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(pfac_ru_rowptr_kernel, dim3(rblocks), dim3(256), 0, s.stream, sorted, (unsigned long long)E,
                           (unsigned long long)n_docs, rbits, (const unsigned long long *)s.tc_bal.p, (const unsigned *)s.tc_x.p,
                           (const unsigned long long *)s.gsum.p, (unsigned long long)total, row);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(row, 0, (n_docs + 1) * 8, s.stream));     // no rule fired: every row is empty
    }
    s.ru_row.commit(n_docs + 1, !d_row_ptr_out);
    s.ru_out.commit(total, !d_rules_out);
    return PFAC_OK;
}

int pfac_documents_rules_d2h(pfac_ctx *ctx, int slot, uint64_t *host_row_ptr, uint32_t *host_rules) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const char *me = "pfac_documents_rules_d2h", *pass = "pfac_documents_rules";
    rc = fetch(ctx, s, s.ru_row, me, pass, host_row_ptr, 0, s.ru_row.n, true);
    return rc ? rc : fetch(ctx, s, s.ru_out, me, pass, host_rules, 0, s.ru_out.n, true);
}

// Proximity rules: the rules' upload, the blocks' last A / last B, their carry-in, the memset and the pass queued back to
// back, then the ONE copy back (the OR of all masks and the error word); behind the host's check the copy to a caller's
// buffer.
int pfac_documents_near(pfac_ctx *ctx, int slot, const pfac_record *d_sel, const uint64_t *d_doc_first, uint64_t n_docs,
                        uint32_t flags, const pfac_near_rule *rules, uint32_t n_rules, uint64_t *d_masks_out, uint64_t *any_mask) {
    const std::string fn = "pfac_documents_near";
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!any_mask) return fail(ctx, PFAC_E_ARG, "null argument");
    *any_mask = 0;
    Slot &s = ctx->slots[slot];
    s.nr_out.invalidate();
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (!ctx->gmask.p) return fail(ctx, PFAC_E_STATE, fn + ": no state groups for the uploaded table (pfac_table_set_state_groups)");
    const pfac_record *sel = d_sel;
    const unsigned long long *first = reinterpret_cast<const unsigned long long *>(d_doc_first);
    uint64_t n = 0;
    const bool own = !d_sel && !d_doc_first;
    if (own && flags == PFAC_NEAR_SELECTION) {              // the rules of pfac_documents_term_counts' slot-owned inputs
        if (!s.scanned || s.pending || !s.ll_out.done || s.ll_seq != s.scan_seq || !s.ll_docs)
            return fail(ctx, PFAC_E_STATE, fn + " needs a pfac_records_leftmost_longest_documents since the slot's last scan");
        if (s.last_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
        if (!s.ll_out.own || !s.lld_first.done || !s.lld_first.own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no selection (it went to the caller's buffers; pass those)");
    } else if (own && flags == 0) {
        if (!s.seg_out.done || !s.seg_out.own || !s.seg_first.done || !s.seg_first.own)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot holds no pfac_records_segment result (none yet, or it went to the caller's buffers; pass those)");
        if (s.seg_table != ctx->table_gen) return fail(ctx, PFAC_E_STATE, fn + ": the segment pass ran with an earlier table");
    }
    if ((((uintptr_t)d_sel | (uintptr_t)d_doc_first | (uintptr_t)d_masks_out) & 7))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_sel, d_doc_first and d_masks_out 8 B)");
    if (!own && (!d_sel || !d_doc_first))
        return fail(ctx, PFAC_E_ARG, fn + ": d_sel and d_doc_first are the slot's (both NULL) or the caller's (neither)");
    if (flags > PFAC_NEAR_SELECTION) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 or PFAC_NEAR_SELECTION");
    if (own) {
        const bool picks = flags == PFAC_NEAR_SELECTION;
        rc = (picks ? s.ll_out : s.seg_out).consume(ctx, fn, "records (d_sel)", d_sel, ANY_N, &sel);
        if (rc) return rc;
        rc = (picks ? s.lld_first : s.seg_first).consume(ctx, fn, "doc_first (d_doc_first)", d_doc_first, n_docs + 1, &first);
        if (rc) return rc;
        n = picks ? s.ll_out.n : s.seg_out.n;
    }
    if (n_docs >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs must be below 2^32");
    if (n_rules > PFAC_NEAR_MAX_RULES) return fail(ctx, PFAC_E_ARG, fn + ": at most 64 rules per call (run it again for more)");
    if (!rules && n_rules) return fail(ctx, PFAC_E_ARG, fn + ": null rules");
    for (uint32_t r = 0; r < n_rules; r++)
        if (rules[r].flags > PFAC_NEAR_ORDERED || rules[r].reserved)
            return fail(ctx, PFAC_E_ARG, fn + ": rule " + std::to_string(r) + ": flags must be 0 or PFAC_NEAR_ORDERED and reserved 0");
    USE_DEVICE(ctx);
    if (!own) {                                             // how many records the caller's arrays hold: doc_first[n_docs]
        HIP_TRY(ctx, hipMemcpyAsync(s.h_ctl + H_PASS, first + n_docs, 8, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(ctx, hipStreamSynchronize(s.stream));
        n = host_u64(s, H_PASS);
    }
    if (n >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": the record count, d_doc_first[n_docs], must be below 2^32");
    const char *broken = ": d_doc_first must start at 0 and not decrease, every state of d_sel must be below num_final, and no position may decrease inside a document";
    if (n_docs == 0 && n) return fail(ctx, PFAC_E_ARG, fn + broken);
    const unsigned n_blocks = (unsigned)((n + NR_BLOCK - 1) / NR_BLOCK);
    rc = ensure_gsum(ctx, s, 1);                            // the OR of all masks, the error word
    if (rc) return rc;
    unsigned long long *res = s.gsum.p;
    // The masks are made in the slot's buffer and reach a caller's only behind the host's check of the error word: a
    // refused call leaves the caller's buffer as it was.
    unsigned long long *out;
    rc = s.nr_out.bind(ctx, s.stream, (unsigned long long *)nullptr, std::max<uint64_t>(n_docs, 1), docs_cap(n_docs), &out);
    if (!rc && n_rules) rc = s.nr_rules.ensure(ctx, s.stream, n_rules, PFAC_NEAR_MAX_RULES);
    const uint64_t tab_n = (uint64_t)n_blocks * n_rules * 2;
    if (!rc && tab_n) rc = s.nr_tab.ensure(ctx, s.stream, tab_n, quarter_more(tab_n));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
    if (n_docs) {
        const unsigned num_final = (unsigned)ctx->plan.base.num_final;
        HIP_TRY(ctx, hipMemsetAsync(out, 0, n_docs * 8, s.stream));      // the 0 of every document in which no rule fired
        if (n_rules) {
            memcpy(s.nr_host, rules, (size_t)n_rules * sizeof(pfac_near_rule));
            HIP_TRY(ctx, hipMemcpyAsync(s.nr_rules.p, s.nr_host, (size_t)n_rules * sizeof(pfac_near_rule), hipMemcpyHostToDevice, s.stream));
        }
        if (tab_n) {
            hipLaunchKernelGGL(pfac_near_last_kernel, dim3((n_blocks + 3) / 4), dim3(256), 0, s.stream, sel, (unsigned long long)n,
                               (const unsigned long long *)ctx->gmask.p, num_final, (const pfac_near_rule *)s.nr_rules.p, (unsigned)n_rules,
                               n_blocks, s.nr_tab.p);
            hipLaunchKernelGGL(pfac_near_carry_kernel, dim3(2 * n_rules), dim3(256), 0, s.stream, s.nr_tab.p, n_blocks);
        }
        const uint64_t vblocks = (n_docs + 255) / 256;
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::max<uint64_t>((n_blocks + 3) / 4, std::min<uint64_t>(vblocks, 4096)));
        hipLaunchKernelGGL(pfac_near_kernel, dim3(blocks), dim3(256), 0, s.stream, sel, (unsigned long long)n, first,
                           (unsigned long long)n_docs, (const unsigned long long *)ctx->gmask.p, num_final,
                           (const pfac_near_rule *)s.nr_rules.p, (unsigned)n_rules, n_blocks, (const unsigned long long *)s.nr_tab.p, out, res);
    }
    rc = pass_words(ctx, s, res, 2);
    if (rc) return rc;
    if (host_u64(s, H_PASS1)) return fail(ctx, PFAC_E_ARG, fn + broken);
    if (d_masks_out && n_docs) HIP_TRY(ctx, hipMemcpyAsync(d_masks_out, out, n_docs * 8, hipMemcpyDeviceToDevice, s.stream));
    *any_mask = host_u64(s, H_PASS);
    s.nr_out.commit(n_docs, !d_masks_out);
    return PFAC_OK;
}

int pfac_near_masks_d2h(pfac_ctx *ctx, int slot, uint64_t *host_masks, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.nr_out, "pfac_near_masks_d2h", "pfac_documents_near", host_masks, first, n);
}

void *pfac_slot_near_masks(pfac_ctx *ctx, int slot) {
    if (check_slot(ctx, slot)) return nullptr;
    const Slot &s = ctx->slots[slot];
    return s.nr_out.done && s.nr_out.own ? (void *)s.nr_out.buf.p : nullptr;
}

// The two gathers: the plain one (fmt NULL, or a format that asks for nothing: the plain kernels) and the one with
// labels.  One pass: one slot-owned output, one slot-owned offset array, one lifetime.
static int ga_run(pfac_ctx *ctx, int slot, const std::string &fn, const void *d_input, uint64_t n_bytes, const uint64_t *d_doc_offsets,
                  uint64_t n_docs, const uint64_t *d_ids, uint64_t n_ids, const uint64_t *d_doc_first, const pfac_line_format *fmt,
                  void *d_out, uint64_t out_cap, uint64_t *d_out_offsets, uint64_t *out_bytes) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out_bytes) return fail(ctx, PFAC_E_ARG, "null argument");
    *out_bytes = 0;
    Slot &s = ctx->slots[slot];
    s.ga_out.invalidate();
    s.ga_off.invalidate();
    if (n_bytes > (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_bytes must be at most 2^32");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    if (!d_input && n_bytes > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": n_bytes exceeds the slot's input buffer");
    const unsigned long long *off = reinterpret_cast<const unsigned long long *>(d_doc_offsets);
    if (!off) {
        if (!s.doc.done || n_docs + 1 != s.doc.n)
            return fail(ctx, PFAC_E_STATE, fn + ": the slot has no document offsets for this n_docs (pfac_slot_doc_offsets)");
        off = s.doc.buf.p;
    }
    const unsigned long long *ids;
    rc = s.dm_out.consume(ctx, fn, "ids of a pfac_documents_matching (n_ids of them)", d_ids, n_ids, &ids);
    if (rc) return rc;
    if (n_docs >= (1ull << 32) || n_ids >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_docs and n_ids must be below 2^32");
    if (((uintptr_t)in | (uintptr_t)d_out) & 15) return fail(ctx, PFAC_E_ARG, fn + ": d_input and d_out must be 16-byte aligned");
    if (((uintptr_t)off | (uintptr_t)ids | (uintptr_t)d_out_offsets) & 7)
        return fail(ctx, PFAC_E_ARG, fn + ": d_doc_offsets, d_ids and d_out_offsets must be 8-byte aligned");
    const bool labels = fmt && (fmt->flags || fmt->group_sep_len);
    GfFormat gf = {};
    const unsigned long long *first = nullptr;
    if (labels) {
        const uint32_t known = PFAC_LINE_NUMBER | PFAC_LINE_OFFSET | PFAC_LINE_TERMINATE | PFAC_LINE_CONTEXT_SEP | PFAC_LINE_SEP_FIRST;
        const uint64_t bound = 1000000000000000000ull;          // of ndigits64
        if (fmt->flags & ~known) return fail(ctx, PFAC_E_ARG, fn + ": unknown flags in the format");
        if (fmt->group_sep_len > PFAC_LINE_MAX_GROUP_SEP) return fail(ctx, PFAC_E_ARG, fn + ": group_sep_len must be at most 8");
        if (fmt->number_base > bound || fmt->number_base + n_docs > bound || fmt->offset_base > bound || fmt->offset_base + n_bytes > bound)
            return fail(ctx, PFAC_E_ARG, fn + ": number_base + n_docs and offset_base + n_bytes must be at most 10^18");
        if (fmt->flags & PFAC_LINE_CONTEXT_SEP) {
            rc = s.seg_first.consume(ctx, fn, "doc_first of a pfac_records_segment (n_docs + 1 entries)", d_doc_first, n_docs + 1, &first);
            if (rc) return rc;
            if ((uintptr_t)first & 7) return fail(ctx, PFAC_E_ARG, fn + ": d_doc_first must be 8-byte aligned");
        }
        gf.flags = fmt->flags;
        gf.sep_len = fmt->group_sep_len;
        gf.chars = (unsigned)fmt->sep_match | (unsigned)fmt->sep_context << 8 | (unsigned)fmt->terminator << 16;
        for (unsigned i = 0; i < gf.sep_len; i++) gf.sep |= (unsigned long long)fmt->group_sep[i] << (8 * i);
        gf.number_base = fmt->number_base;
        gf.offset_base = fmt->offset_base;
    }
    USE_DEVICE(ctx);
    const uint64_t nb = (n_ids + RP_BLOCK - 1) / RP_BLOCK;
    const unsigned n_groups = (unsigned)((nb + RP_GROUP - 1) / RP_GROUP);
    uint64_t total = 0;
    if (n_ids) {
        rc = s.ga_x.ensure(ctx, s.stream, nb, quarter_more(nb));
        if (rc) return rc;
        rc = ensure_gsum(ctx, s, n_groups + 1);             // group prefixes, the total, the error word
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups + 1;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 8, s.stream));
        if (labels)
            hipLaunchKernelGGL(pfac_gf_count_kernel, dim3(n_groups), dim3(RP_GROUP / 4 * WAVE), 0, s.stream, in, ids,
                               (unsigned long long)n_ids, off, (unsigned long long)n_docs, (unsigned long long)n_bytes, gf,
                               s.ga_x.p, s.gsum.p, res);
        else
            hipLaunchKernelGGL(pfac_ga_count_kernel, dim3(n_groups), dim3(RP_GROUP / 4 * WAVE), 0, s.stream, ids,
                               (unsigned long long)n_ids, off, (unsigned long long)n_docs, (unsigned long long)n_bytes, s.ga_x.p,
                               s.gsum.p, res);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
        rc = pass_words(ctx, s, s.gsum.p + n_groups, 2);
        if (rc) return rc;
        if (host_u64(s, H_PASS1))
            return fail(ctx, PFAC_E_ARG, fn + ": every id must be below n_docs, and off[id] <= off[id + 1] <= n_bytes for every selected document");
        total = host_u64(s, H_PASS);
    }
    *out_bytes = total;
    if (d_out && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " output bytes, out_cap is " + std::to_string(out_cap));
    unsigned long long *oo;
    unsigned char *out;
    rc = s.ga_off.bind(ctx, s.stream, d_out_offsets, n_ids + 1, docs_cap(n_ids), &oo);      // (everything allocated before the first write)
    if (!rc) rc = s.ga_out.bind(ctx, s.stream, d_out, total, align_up(total + total / 8, 4096), &out);
    if (rc) return rc;
    if (n_ids) {
        if (labels)
            hipLaunchKernelGGL(pfac_gf_offsets_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(4 * WAVE), 0, s.stream, in, ids,
                               (unsigned long long)n_ids, off, gf, (const unsigned long long *)s.ga_x.p,
                               (const unsigned long long *)s.gsum.p, oo);
        else
            hipLaunchKernelGGL(pfac_ga_offsets_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(4 * WAVE), 0, s.stream, ids,
                               (unsigned long long)n_ids, off, (const unsigned long long *)s.ga_x.p,
                               (const unsigned long long *)s.gsum.p, oo);
        HIP_TRY(ctx, hipGetLastError());
    } else {
        HIP_TRY(ctx, hipMemsetAsync(oo, 0, 8, s.stream));    // no ids: the single offset 0
    }
    if (total) {
        const WriteGrid g = write_grid(total);
        if (labels)
            hipLaunchKernelGGL(pfac_gf_write_kernel, dim3(g.blocks), dim3(RP_WAVES * WAVE), 0, s.stream, in,
                               (unsigned long long)n_bytes, ids, (unsigned long long)n_ids, off, first, gf,
                               (const unsigned long long *)oo, (const unsigned long long *)s.ga_x.p,
                               (const unsigned long long *)s.gsum.p, (unsigned long long)total, g.wins, out);
        else
            hipLaunchKernelGGL(pfac_ga_write_kernel, dim3(g.blocks), dim3(RP_WAVES * WAVE), 0, s.stream, in,
                               (unsigned long long)n_bytes, ids, (unsigned long long)n_ids, off, (const unsigned long long *)oo,
                               (const unsigned long long *)s.ga_x.p, (const unsigned long long *)s.gsum.p, (unsigned long long)total,
                               g.wins, out);
        HIP_TRY(ctx, hipGetLastError());
    }
    s.ga_out.commit(total, !d_out);
    s.ga_off.commit(n_ids + 1, !d_out_offsets);
    return PFAC_OK;
}

int pfac_documents_gather(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, const uint64_t *d_doc_offsets,
                          uint64_t n_docs, const uint64_t *d_ids, uint64_t n_ids, void *d_out, uint64_t out_cap,
                          uint64_t *d_out_offsets, uint64_t *out_bytes) {
    return ga_run(ctx, slot, "pfac_documents_gather", d_input, n_bytes, d_doc_offsets, n_docs, d_ids, n_ids, nullptr, nullptr, d_out,
                  out_cap, d_out_offsets, out_bytes);
}

int pfac_documents_gather_format(pfac_ctx *ctx, int slot, const void *d_input, uint64_t n_bytes, const uint64_t *d_doc_offsets,
                                 uint64_t n_docs, const uint64_t *d_ids, uint64_t n_ids, const uint64_t *d_doc_first,
                                 const pfac_line_format *fmt, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                                 uint64_t *out_bytes) {
    return ga_run(ctx, slot, "pfac_documents_gather_format", d_input, n_bytes, d_doc_offsets, n_docs, d_ids, n_ids, d_doc_first, fmt,
                  d_out, out_cap, d_out_offsets, out_bytes);
}

int pfac_documents_gather_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.ga_out, "pfac_documents_gather_d2h", "pfac_documents_gather", host, first, n);
}

int pfac_documents_gather_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_out_offsets) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.ga_off, "pfac_documents_gather_offsets_d2h", "pfac_documents_gather", host_out_offsets, 0, s.ga_off.n);
}

int pfac_records_filter_words(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, const uint64_t word_set[4],
                              uint32_t edges, int prev_byte, int next_byte, const uint64_t *d_doc_offsets, uint64_t n_docs,
                              uint64_t *n_kept) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_kept) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_kept = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_records_filter_words";
    rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE | SCAN_FITS);
    if (rc) return rc;
    if (edges < 1 || edges > (PFAC_WORD_LEFT | PFAC_WORD_RIGHT)) return fail(ctx, PFAC_E_ARG, fn + ": edges must be PFAC_WORD_LEFT, PFAC_WORD_RIGHT or both");
    if (prev_byte < -1 || prev_byte > 255 || next_byte < -1 || next_byte > 255)
        return fail(ctx, PFAC_E_ARG, fn + ": prev_byte and next_byte must be -1 (no byte) or 0..255");
    void *heap = d_records ? d_records : (void *)s.records.p;
    if (heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    if ((uintptr_t)in & 15) return fail(ctx, PFAC_E_ARG, fn + ": d_input must be 16-byte aligned");
    if (!d_input && s.last_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
    if (!in && s.last_total) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    const unsigned long long *off = nullptr;
    if (n_docs && !d_doc_offsets && (!s.doc.done || n_docs + 1 != s.doc.n))
        return fail(ctx, PFAC_E_STATE, fn + ": the slot has no document offsets for this n_docs (pfac_slot_doc_offsets)");
    rc = n_docs ? resolve_docs(ctx, s, fn, d_doc_offsets, n_docs, 0, &off) : PFAC_OK;
    if (rc) return rc;
    WordSet ws;
    for (int k = 0; k < 4; k++)                              // NULL: [0-9A-Za-z_]
        ws.w[k] = word_set ? word_set[k] : (k == 0 ? 0x03FF000000000000ull : (k == 1 ? 0x07FFFFFE87FFFFFEull : 0ull));
    USE_DEVICE(ctx);
    const uint64_t n_tiles = s.last_tiles;
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, 1);                            // the kept total and the offsets' error flag
    if (rc) return rc;
    unsigned long long *res = s.gsum.p;
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
    if (n_docs) launch_offsets_check(s, off, n_docs, res + 1);          // in front of the filter
    if (n_groups) {
        const bool dk = n_docs != 0;
        auto fk = by_width(s.last_rec_bytes, [dk](auto w) { return dk ? pfac_filter_words_kernel<w(), true> : pfac_filter_words_kernel<w(), false>; });
        hipLaunchKernelGGL(fk, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, heap, s.tile_index.p, (unsigned long long)n_tiles,
                           (unsigned long long)s.last_cap, in, (unsigned long long)s.last_avail, ctx->flen.p, (unsigned)ctx->plan.base.num_final,
                           ws, (unsigned)edges, prev_byte, next_byte, off, (unsigned long long)n_docs,
                           (const unsigned long long *)(res + 1), res);
    }
    rc = pass_words(ctx, s, res, 2);
    if (rc) return rc;
    if (host_u64(s, H_PASS1)) return bad_doc_offsets(ctx, s, fn);
    // the kept records ARE the scan's records from here on: its match count (a repeated pfac_scan_finish reads it from
    // the result words), and a new record set for whatever selected from the old one
    const uint64_t total = host_u64(s, H_PASS);
    s.last_total = total;
    s.h_ctl[H_MATCHES] = (unsigned)total;
    s.h_ctl[H_MATCHES + 1] = (unsigned)(total >> 32);
    s.scan_seq++;
    *n_kept = total;
    return PFAC_OK;
}

int pfac_table_set_state_spans(pfac_ctx *ctx, const pfac_state_span *spans, uint64_t n_states) {
    static_assert(sizeof(pfac_state_span) == sizeof(uint4), "a span is one dwordx4");
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "pfac_table_set_state_spans before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!spans && n_states))
        return fail(ctx, PFAC_E_ARG, "pfac_table_set_state_spans: need num_final spans (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    for (uint64_t i = 0; i < n_states; i++)
        if (spans[i].reserved)
            return fail(ctx, PFAC_E_ARG, "pfac_table_set_state_spans: reserved must be 0 (final state " + std::to_string(i) + ")");
    USE_DEVICE(ctx);
    // as the state groups: a buffer of its own for every call, built aside; freeing the old one waits for the device --
    // a filter that still reads the old spans has finished before they go
    DevBuf<uint4> fresh;
    const uint64_t n = std::max<uint64_t>(n_states, 1);
    int rc = fresh.ensure(ctx, nullptr, n, n);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(fresh.p, 0xFF, n * sizeof(uint4)));
    if (n_states) HIP_TRY(ctx, hipMemcpy(fresh.p, spans, n_states * sizeof(uint4), hipMemcpyHostToDevice));
    ctx->spans = std::move(fresh);
    return PFAC_OK;
}

int pfac_records_filter_spans(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, int delimiter, uint32_t flags,
                              const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t *n_kept) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_kept) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_kept = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_records_filter_spans";
    rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    const bool line = (flags & PFAC_SPANS_LINE) != 0;
    if (!line && !ctx->spans.p) return fail(ctx, PFAC_E_STATE, fn + ": no state spans for the uploaded table (pfac_table_set_state_spans)");
    if (n_docs && !d_doc_offsets && (!s.doc.done || n_docs + 1 != s.doc.n))
        return fail(ctx, PFAC_E_STATE, fn + ": the slot has no document offsets for this n_docs (pfac_slot_doc_offsets, pfac_slot_doc_offsets_split)");
    rc = last_scan_usable(ctx, s, fn, SCAN_FITS);
    if (rc) return rc;
    if (delimiter < -1 || delimiter > 255) return fail(ctx, PFAC_E_ARG, fn + ": delimiter must be -1 (none) or 0..255");
    if (flags > PFAC_SPANS_LINE) return fail(ctx, PFAC_E_ARG, fn + ": flags must be 0 or PFAC_SPANS_LINE");
    void *heap = d_records ? d_records : (void *)s.records.p;
    if (heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    const unsigned char *in = nullptr;                       // no delimiter: the input is never read
    if (delimiter >= 0) {
        in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
        if ((uintptr_t)in & 15) return fail(ctx, PFAC_E_ARG, fn + ": d_input must be 16-byte aligned");
        if (!d_input && s.last_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
        if (!in && s.last_total) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    }
    const unsigned long long *off = nullptr;
    rc = n_docs ? resolve_docs(ctx, s, fn, d_doc_offsets, n_docs, 0, &off) : PFAC_OK;
    if (rc) return rc;
    USE_DEVICE(ctx);
    const uint64_t n_tiles = s.last_tiles;
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, 1);                            // the kept total and the offsets' error flag
    if (rc) return rc;
    unsigned long long *res = s.gsum.p;
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
    if (n_docs) launch_offsets_check(s, off, n_docs, res + 1);          // in front of the filter
    if (n_groups) {
        const bool dk = n_docs != 0;
        auto fk = by_width(s.last_rec_bytes, [dk, line](auto w) {
            return dk ? (line ? pfac_filter_spans_kernel<w(), true, true> : pfac_filter_spans_kernel<w(), true, false>)
                      : (line ? pfac_filter_spans_kernel<w(), false, true> : pfac_filter_spans_kernel<w(), false, false>);
        });
        hipLaunchKernelGGL(fk, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, heap, s.tile_index.p, (unsigned long long)n_tiles,
                           (unsigned long long)s.last_cap, in, (unsigned long long)s.last_avail, ctx->flen.p,
                           (const uint4 *)(line ? nullptr : ctx->spans.p), (unsigned)ctx->plan.base.num_final, delimiter, off,
                           (unsigned long long)n_docs, (const unsigned long long *)(res + 1), res);
    }
    rc = pass_words(ctx, s, res, 2);
    if (rc) return rc;
    if (host_u64(s, H_PASS1)) return bad_doc_offsets(ctx, s, fn);
    // as after the whole-word filter: the kept records ARE the scan's records from here on
    const uint64_t total = host_u64(s, H_PASS);
    s.last_total = total;
    s.h_ctl[H_MATCHES] = (unsigned)total;
    s.h_ctl[H_MATCHES + 1] = (unsigned)(total >> 32);
    s.scan_seq++;
    *n_kept = total;
    return PFAC_OK;
}

// The documents of a per-document selection, as the caller passed them (NULL: the slot's offsets / a slot-owned
// doc_first); ll_select without them makes the plain selection.
struct LlDocs {
    const uint64_t *off;
    uint64_t n_docs;
    uint64_t *first;
};

// pfac_records_leftmost_longest, and with `docs` pfac_records_leftmost_longest_documents (entry 0): the same kernels,
// the tile passes in their document form, and the document write.
static int ll_select(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_records, uint32_t entry, pfac_record *d_out,
                     uint64_t out_cap, uint64_t *n_selected, uint32_t *exit_offset, const LlDocs *docs) {
    s.ll_out.invalidate();
    s.lld_first.invalidate();
    int rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    // (PFAC_E_STATE, as pfac.h documents for the selections; the other passes report PFAC_E_OVERFLOW)
    if (s.last_used > s.last_cap) return fail(ctx, PFAC_E_STATE, fn + ": the slot's last scan overflowed its record heap");
    const unsigned M = (unsigned)ctx->plan.max_pat_len;
    if (entry > M) return fail(ctx, PFAC_E_ARG, fn + ": entry " + std::to_string(entry) + " exceeds max_pat_len " + std::to_string(M));
    const int rb = s.last_rec_bytes;
    const void *src = d_records ? d_records : s.records.p;
    if (((uintptr_t)d_out & 7) || ((uintptr_t)src & (uintptr_t)(rb - 1)))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_out 8 B, records their width)");
    if (!src && s.last_tiles) return fail(ctx, PFAC_E_ARG, "null record buffer");
    const unsigned long long *off = nullptr;
    const uint64_t n_docs = docs ? docs->n_docs : 0;
    rc = docs ? resolve_docs(ctx, s, fn, docs->off, n_docs, (uintptr_t)docs->first, &off) : PFAC_OK;
    if (rc) return rc;
    USE_DEVICE(ctx);
    const uint64_t n_tiles = s.last_tiles;
    unsigned long long *first = nullptr;
    auto done = [&](uint64_t total, uint32_t ex) {
        s.ll_seq = s.scan_seq;
        s.ll_entry = entry;
        s.ll_exit = ex;
        s.ll_docs = docs != nullptr;
        if (docs) {
            s.lld_gen = s.doc_gen;
            s.lld_own_off = docs->off == nullptr;
            s.lld_first.commit(n_docs + 1, !docs->first);
        }
        s.ll_out.commit(total, !d_out);
        return PFAC_OK;
    };
    if (n_tiles == 0) {                                     // nothing scanned: nothing picked, the cursor stays
        if (!docs) return done(0, entry);
        // every document is empty: check the offsets (no tiles: n_owned is 0), then doc_first = 0
        rc = ensure_gsum(ctx, s, 1);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(s.gsum.p, 0, 8, s.stream));
        launch_offsets_check(s, off, n_docs, s.gsum.p);
        rc = pass_words(ctx, s, s.gsum.p, 1, H_PASS1);
        if (rc) return rc;
        if (host_u64(s, H_PASS1)) return bad_doc_offsets(ctx, s, fn);
        rc = s.lld_first.bind(ctx, s.stream, docs->first, n_docs + 1, docs_cap(n_docs), &first);
        if (rc) return rc;
        HIP_TRY(ctx, hipMemsetAsync(first, 0, (n_docs + 1) * 8, s.stream));
        return done(0, entry);
    }
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP), nb = (n_groups + XGROUP - 1) / XGROUP;
    const unsigned M1 = M + 1, FS = ll_fun_stride(M1);
    // scratch: G_g, the composed functions of 64 groups, their entries, the groups' entries, picks per tile, bitmaps
    const size_t o_gfun = 0, o_hfun = align_up(o_gfun + (size_t)n_groups * FS * 2, 256);
    const size_t o_hat = align_up(o_hfun + (size_t)nb * FS * 2, 256), o_gat = align_up(o_hat + (size_t)nb * 2, 256);
    const size_t o_tcnt = align_up(o_gat + (size_t)n_groups * 2, 256), o_bits = align_up(o_tcnt + n_tiles * 4, 256);
    const size_t need = o_bits + n_tiles * (WTILE / 8);
    rc = s.ll_tmp.ensure(ctx, s.stream, need, need + need / 4);
    if (rc) return rc;
    unsigned short *gfun = reinterpret_cast<unsigned short *>(s.ll_tmp.p + o_gfun), *hfun = reinterpret_cast<unsigned short *>(s.ll_tmp.p + o_hfun);
    unsigned short *hat = reinterpret_cast<unsigned short *>(s.ll_tmp.p + o_hat), *gat = reinterpret_cast<unsigned short *>(s.ll_tmp.p + o_gat);
    unsigned *tcnt = reinterpret_cast<unsigned *>(s.ll_tmp.p + o_tcnt);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(s.ll_tmp.p + o_bits);
    rc = ensure_gsum(ctx, s, n_groups + 2);                 // group prefixes, the total, the exit offset, the offsets' error word
    if (rc) return rc;
    unsigned long long *bad = docs ? s.gsum.p + n_groups + 2 : nullptr;
    if (docs) HIP_TRY(ctx, hipMemsetAsync(bad, 0, 8, s.stream));
    const bool dk = docs != nullptr;
    auto fk = by_width(rb, [dk](auto w) { return dk ? pfac_ll_tiles_kernel<w(), false, true> : pfac_ll_tiles_kernel<w(), false, false>; });
    auto mk = by_width(rb, [dk](auto w) { return dk ? pfac_ll_tiles_kernel<w(), true, true> : pfac_ll_tiles_kernel<w(), true, false>; });
    const size_t lds = ll_tiles_lds(M1);
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)fk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)mk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned long long nt = n_tiles, cap = s.last_cap, own = s.last_owned, nd = n_docs;
    hipLaunchKernelGGL(fk, dim3(n_groups), dim3(LL_WAVES * WAVE), lds, s.stream, src, s.tile_index.p, nt, cap, own, ctx->flen.p,
                       (unsigned)ctx->plan.base.num_final, M, gfun, (const unsigned short *)nullptr, bits, tcnt, s.gsum.p, off, nd, bad);
    hipLaunchKernelGGL(pfac_ll_compose_kernel, dim3(nb), dim3(1024), LL_CHUNK_BYTES, s.stream, gfun, M1, n_groups, (unsigned)XGROUP, hfun);
    hipLaunchKernelGGL(pfac_ll_walk_kernel, dim3(1), dim3(256), LL_CHUNK_BYTES, s.stream, hfun, M1, nb, nb, (const unsigned short *)nullptr,
                       (unsigned)entry, hat, s.gsum.p + n_groups + 1);
    hipLaunchKernelGGL(pfac_ll_walk_kernel, dim3(nb), dim3(256), LL_CHUNK_BYTES, s.stream, gfun, M1, n_groups, (unsigned)XGROUP,
                       (const unsigned short *)hat, 0u, gat, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(mk, dim3(n_groups), dim3(LL_WAVES * WAVE), lds, s.stream, src, s.tile_index.p, nt, cap, own, ctx->flen.p,
                       (unsigned)ctx->plan.base.num_final, M, (unsigned short *)nullptr, (const unsigned short *)gat, bits, tcnt, s.gsum.p,
                       off, nd, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, n_groups);
    rc = pass_words(ctx, s, s.gsum.p + n_groups, docs ? 3 : 2);
    if (rc) return rc;
    const uint64_t total = host_u64(s, H_PASS);
    if (docs) {
        if (host_u64(s, H_PASS2)) return bad_doc_offsets(ctx, s, fn);
        if (s.h_ctl[H_PASS1]) return fail(ctx, PFAC_E_INTERNAL, fn + ": a pick ran past the last document");
    }
    *n_selected = total;
    *exit_offset = s.h_ctl[H_PASS1];
    if (d_out && total > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(total) + " records selected, out_cap is " + std::to_string(out_cap));
    pfac_record *out;
    rc = s.ll_out.bind(ctx, s.stream, d_out, total, total + total / 8 + 4096, &out);
    if (rc) return rc;
    if (docs) {
        rc = s.lld_first.bind(ctx, s.stream, docs->first, n_docs + 1, docs_cap(n_docs), &first);
        if (rc) return rc;
        auto wk = by_width(rb, [](auto w) { return pfac_ll_doc_write_kernel<w()>; });
        hipLaunchKernelGGL(wk, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, src, s.tile_index.p, nt, cap, off, nd, ctx->flen.p,
                           (unsigned)ctx->plan.base.num_final, bits, tcnt, s.gsum.p, n_groups, out, first);
        HIP_TRY(ctx, hipGetLastError());
    } else if (total) {
        auto wk = by_width(rb, [](auto w) { return pfac_ll_write_kernel<w()>; });
        hipLaunchKernelGGL(wk, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, src, s.tile_index.p, nt, cap, bits, tcnt, s.gsum.p,
                           n_groups, out);
        HIP_TRY(ctx, hipGetLastError());
    }
    return done(total, *exit_offset);
}

int pfac_records_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_records, uint32_t entry, pfac_record *d_out,
                                  uint64_t out_cap, uint64_t *n_selected, uint32_t *exit_offset) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_selected || !exit_offset) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_selected = 0;
    *exit_offset = entry;
    return ll_select(ctx, ctx->slots[slot], "pfac_records_leftmost_longest", d_records, entry, d_out, out_cap, n_selected,
                     exit_offset, nullptr);
}

int pfac_records_leftmost_longest_documents(pfac_ctx *ctx, int slot, const void *d_records, const uint64_t *d_doc_offsets,
                                            uint64_t n_docs, pfac_record *d_out, uint64_t out_cap, uint64_t *d_doc_first,
                                            uint64_t *n_selected) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_selected) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_selected = 0;
    uint32_t ex = 0;
    const LlDocs docs{d_doc_offsets, n_docs, d_doc_first};
    return ll_select(ctx, ctx->slots[slot], "pfac_records_leftmost_longest_documents", d_records, 0, d_out, out_cap, n_selected,
                     &ex, &docs);
}

int pfac_leftmost_longest_d2h(pfac_ctx *ctx, int slot, pfac_record *host) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.ll_out, "pfac_leftmost_longest_d2h", "pfac_records_leftmost_longest", host, 0, s.ll_out.n);
}

int pfac_leftmost_longest_documents_d2h(pfac_ctx *ctx, int slot, pfac_record *host_records, uint64_t *host_doc_first) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const char *fn = "pfac_leftmost_longest_documents_d2h", *pass = "pfac_records_leftmost_longest_documents";
    if (!s.ll_docs) return fail(ctx, PFAC_E_STATE, std::string(fn) + " without a finished " + pass);   // (the last selection was a plain one)
    rc = fetch(ctx, s, s.ll_out, fn, pass, host_records, 0, s.ll_out.n, true);
    return rc ? rc : fetch(ctx, s, s.lld_first, fn, pass, host_doc_first, 0, s.lld_first.n, true);
}

// Both setters of the replacements: everything is checked first, the new buffers are made aside and take the place of the
// old ones together, so a refused call leaves the earlier replacements and splits in force.  The old buffers are freed
// behind that (hipFree waits for the device: a write kernel that still reads them has finished before they go), as the
// spans and the groups are.
static int set_replacements(pfac_ctx *ctx, const std::string &fn, const uint32_t *offsets, const uint32_t *splits,
                            uint64_t n_states, const void *bytes, uint64_t n_bytes) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || !offsets || (!bytes && n_bytes))
        return fail(ctx, PFAC_E_ARG, fn + ": need num_final + 1 offsets (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    if (n_bytes >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": n_bytes must be below 2^32");
    bool quoting = false;
    for (uint64_t i = 0; i < n_states; i++) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] > n_bytes)
            return fail(ctx, PFAC_E_ARG, fn + ": offsets must ascend within n_bytes (final state " + std::to_string(i) + ")");
        if (offsets[i + 1] - offsets[i] > PFAC_MAX_REPLACEMENT)
            return fail(ctx, PFAC_E_ARG, fn + ": the replacement of final state " + std::to_string(i) + " exceeds " +
                                             std::to_string(PFAC_MAX_REPLACEMENT) + " bytes");
        if (splits && splits[i] != PFAC_TEMPLATE_PLAIN) {
            if (splits[i] > offsets[i + 1] - offsets[i])
                return fail(ctx, PFAC_E_ARG, fn + ": the split of final state " + std::to_string(i) + " lies past its replacement");
            quoting = true;
        }
    }
    USE_DEVICE(ctx);
    DevBuf<unsigned> off, split;
    DevBuf<unsigned char> rep;
    const uint64_t size = align_up(n_bytes, 16) + 16;
    int rc = off.ensure(ctx, nullptr, n_states + 1, n_states + 1);
    if (!rc) rc = rep.ensure(ctx, nullptr, size, size);
    if (!rc && quoting) rc = split.ensure(ctx, nullptr, n_states, n_states);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(rep.p, 0, size));
    HIP_TRY(ctx, hipMemcpy(off.p, offsets, (n_states + 1) * 4, hipMemcpyHostToDevice));
    if (n_bytes) HIP_TRY(ctx, hipMemcpy(rep.p, bytes, n_bytes, hipMemcpyHostToDevice));
    if (quoting) HIP_TRY(ctx, hipMemcpy(split.p, splits, n_states * 4, hipMemcpyHostToDevice));
    ctx->rep_off = std::move(off);                          // (a swap: the old buffers go with the three locals)
    ctx->rep = std::move(rep);
    ctx->rep_split = std::move(split);
    return PFAC_OK;
}

int pfac_table_set_replacements(pfac_ctx *ctx, const uint32_t *offsets, uint64_t n_states, const void *bytes, uint64_t n_bytes) {
    return set_replacements(ctx, "pfac_table_set_replacements", offsets, nullptr, n_states, bytes, n_bytes);
}

int pfac_table_set_replacement_templates(pfac_ctx *ctx, const uint32_t *offsets, const uint32_t *splits, uint64_t n_states,
                                         const void *bytes, uint64_t n_bytes) {
    return set_replacements(ctx, "pfac_table_set_replacement_templates", offsets, splits, n_states, bytes, n_bytes);
}

// The documents of pfac_replace_documents as the caller passed them (NULL: the slot's offsets / doc_first of the
// selection, the slot-owned output offsets); rp_run without them is pfac_replace_leftmost_longest.
struct RpDocs {
    const uint64_t *off, *first;
    uint64_t *out_off;
};
// pfac_extract_leftmost_longest: the caller's pick offsets (NULL: the slot-owned ones).  rp_run with it writes the picks
// alone, into the extraction's own outputs; the replace's stay as they are, and the reverse.
struct RpExtract {
    uint64_t *pick_off;
};

// f(kernel<TEMPLATES, GAPS>) for the instantiation a call runs: TEMPLATES while some state quotes its match, GAPS
// unless the call is the extraction
#define RP_KERNEL(name, tpl, gaps)                                                                          \
    ((tpl) ? ((gaps) ? name<true, true> : name<true, false>) : ((gaps) ? name<false, true> : name<false, false>))

static int rp_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_input, const pfac_record *d_sel, void *d_out,
                  uint64_t out_cap, uint64_t *out_bytes, const RpDocs *docs, const RpExtract *ext = nullptr) {
    PassOut<unsigned char> &bytes_out = ext ? s.ex_out : s.rp_out;
    bytes_out.invalidate();
    if (ext) s.ex_off.invalidate();
    else s.rpd_off.invalidate();
    if (!s.scanned || !s.ll_out.done || s.ll_seq != s.scan_seq || (docs && !s.ll_docs))
        return fail(ctx, PFAC_E_STATE, fn + (docs ? " needs a pfac_records_leftmost_longest_documents since the slot's last scan"
                                                  : " needs a pfac_records_leftmost_longest since the slot's last scan"));
    if (!ctx->have_table || s.last_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
    if (!ctx->rep.p) return fail(ctx, PFAC_E_STATE, fn + ": no replacements for the uploaded table (pfac_table_set_replacements)");
    if (!ctx->flen.p) return fail(ctx, PFAC_E_STATE, fn + ": no final-state lengths for the uploaded table");
    const pfac_record *sel;
    int rc = s.ll_out.consume(ctx, fn, "selection (d_sel)", d_sel, ANY_N, &sel);
    if (rc) return rc;
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    const uint64_t n = s.ll_out.n, n_owned = s.last_owned, n_avail = s.last_avail, entry = s.ll_entry, ex = s.ll_exit;
    if (((uintptr_t)d_out & 15) || ((uintptr_t)in & 15) || ((uintptr_t)d_sel & 7) || (ext && ((uintptr_t)ext->pick_off & 7)))
        return fail(ctx, PFAC_E_ARG, fn + (ext ? ": misaligned buffer (d_input and d_out 16 B, d_sel and d_pick_offsets 8 B)"
                                               : ": misaligned buffer (d_input and d_out 16 B, d_sel 8 B)"));
    if (n_owned > entry && !in) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    if (!d_input && n_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
    const unsigned long long *doff = nullptr, *dfirst = nullptr;
    unsigned long long *dout_off = nullptr;
    if (docs) {
        doff = reinterpret_cast<const unsigned long long *>(docs->off);
        dout_off = reinterpret_cast<unsigned long long *>(docs->out_off);
        if (!doff) {
            if (!s.lld_own_off) return fail(ctx, PFAC_E_STATE, fn + ": the selection cut the caller's document offsets; pass them as d_doc_offsets");
            if (s.lld_gen != s.doc_gen || !s.doc.done) return fail(ctx, PFAC_E_STATE, fn + ": the slot's document offsets changed since the selection");
            doff = s.doc.buf.p;
        }
        rc = s.lld_first.consume(ctx, fn, "doc_first of the selection (d_doc_first)", docs->first, ANY_N, &dfirst);
        if (rc) return rc;
        if (((uintptr_t)doff & 7) || ((uintptr_t)dfirst & 7) || ((uintptr_t)dout_off & 7))
            return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    }
    USE_DEVICE(ctx);
    const bool tpl = ctx->rep_split.p != nullptr, gaps = !ext;
    int64_t delta = 0;
    const uint64_t nb = n ? (n + RP_BLOCK - 1) / RP_BLOCK : 1;
    const uint64_t n_groups = (nb + RP_GROUP - 1) / RP_GROUP;
    if (n_groups >= (1ull << 32)) return fail(ctx, PFAC_E_ARG, fn + ": too many picks");
    unsigned long long *X = nullptr;
    if (n) {
        const size_t need = nb * 8;
        rc = s.rp_tmp.ensure(ctx, s.stream, need, need + need / 4 + 4096);
        if (rc) return rc;
        X = reinterpret_cast<unsigned long long *>(s.rp_tmp.p);
        rc = ensure_gsum(ctx, s, (unsigned)n_groups + 2);       // group prefixes, the total delta, error flag, c_{n-1}
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups + 1;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        hipLaunchKernelGGL(RP_KERNEL(pfac_rp_count_kernel, tpl, gaps), dim3((unsigned)n_groups), dim3(RP_GROUP / 4 * WAVE), 0,
                           s.stream, sel, (unsigned long long)n, (unsigned long long)entry, (unsigned long long)n_owned,
                           ctx->flen.p, ctx->rep_off.p, (unsigned)ctx->plan.base.num_final, X, s.gsum.p, res,
                           (const unsigned *)ctx->rep_split.p);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, (unsigned)n_groups);
        rc = pass_words(ctx, s, s.gsum.p + n_groups, 3);
        if (rc) return rc;
        delta = (int64_t)host_u64(s, H_PASS);
        const uint64_t err = host_u64(s, H_PASS1), c_last = host_u64(s, H_PASS2);
        if (err || (c_last > n_owned ? c_last - n_owned : 0) != ex)
            return fail(ctx, PFAC_E_ARG, fn + ": the selection is not one of this scan and table");
    }
    const int64_t total = ext ? delta : (int64_t)(n_owned + ex) - (int64_t)entry + delta;    // (the picks alone: the sum of their lengths)
    if (total < 0) return fail(ctx, PFAC_E_INTERNAL, fn + ": negative output length");
    const uint64_t ob = (uint64_t)total;
    *out_bytes = ob;
    if (d_out && ob > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(ob) + " output bytes, out_cap is " + std::to_string(out_cap));
    const uint64_t n_docs = docs ? s.lld_first.n - 1 : 0;
    unsigned long long *oo = nullptr;
    if (docs) {                                             // (everything allocated before the first write)
        rc = s.rpd_off.bind(ctx, s.stream, dout_off, n_docs + 1, docs_cap(n_docs), &oo);
        if (!rc && n) rc = s.rpd_tmp.ensure(ctx, s.stream, n + 1, n + 1 + n / 8 + 4096);
        if (rc) return rc;
    }
    unsigned long long *po = nullptr;
    if (ext) {
        rc = s.ex_off.bind(ctx, s.stream, ext->pick_off, n + 1, docs_cap(n), &po);
        if (rc) return rc;
    }
    unsigned char *out;
    rc = bytes_out.bind(ctx, s.stream, d_out, ob, align_up(ob + ob / 8, 4096), &out);
    if (rc) return rc;
    if (ob) {
        const WriteGrid g = write_grid(ob);
        hipLaunchKernelGGL(RP_KERNEL(pfac_rp_write_kernel, tpl, gaps), dim3(g.blocks), dim3(RP_WAVES * WAVE), 0, s.stream, in,
                           (unsigned long long)n_avail, sel, (unsigned long long)n, (unsigned long long)entry, ctx->flen.p,
                           ctx->rep_off.p, ctx->rep.p, (unsigned long long)ctx->rep.cap, X, s.gsum.p,
                           (unsigned long long)ob, g.wins, out, (const unsigned *)ctx->rep_split.p);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (ext) {                                              // the pick offsets: D_k of the delta kernel as they come
        if (n)
            hipLaunchKernelGGL(RP_KERNEL(pfac_rp_doc_delta_kernel, tpl, false), dim3((unsigned)((nb + 3) / 4)), dim3(4 * WAVE), 0,
                               s.stream, sel, (unsigned long long)n, ctx->flen.p, ctx->rep_off.p, X, s.gsum.p, po,
                               (const unsigned *)ctx->rep_split.p);
        else
            HIP_TRY(ctx, hipMemsetAsync(po, 0, 8, s.stream));
        HIP_TRY(ctx, hipGetLastError());
        s.ex_off.commit(n + 1, !ext->pick_off);
    }
    if (docs) {
        if (n)
            hipLaunchKernelGGL(RP_KERNEL(pfac_rp_doc_delta_kernel, tpl, true), dim3((unsigned)((nb + 3) / 4)), dim3(4 * WAVE), 0,
                               s.stream, sel, (unsigned long long)n, ctx->flen.p, ctx->rep_off.p, X, s.gsum.p, s.rpd_tmp.p,
                               (const unsigned *)ctx->rep_split.p);
        const unsigned oblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 1 + 255) / 256, 65536));
        hipLaunchKernelGGL(pfac_rp_doc_offsets_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, dfirst,
                           (unsigned long long)n_docs, (const unsigned long long *)s.rpd_tmp.p, (unsigned long long)n, oo);
        HIP_TRY(ctx, hipGetLastError());
        s.rpd_off.commit(n_docs + 1, !dout_off);
    }
    bytes_out.commit(ob, !d_out);
    return PFAC_OK;
}

int pfac_replace_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, void *d_out,
                                  uint64_t out_cap, uint64_t *out_bytes) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out_bytes) return fail(ctx, PFAC_E_ARG, "null argument");
    *out_bytes = 0;
    return rp_run(ctx, ctx->slots[slot], "pfac_replace_leftmost_longest", d_input, d_sel, d_out, out_cap, out_bytes, nullptr);
}

int pfac_replace_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                           const uint64_t *d_doc_first, void *d_out, uint64_t out_cap, uint64_t *d_out_offsets, uint64_t *out_bytes) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out_bytes) return fail(ctx, PFAC_E_ARG, "null argument");
    *out_bytes = 0;
    const RpDocs docs{d_doc_offsets, d_doc_first, d_out_offsets};
    return rp_run(ctx, ctx->slots[slot], "pfac_replace_documents", d_input, d_sel, d_out, out_cap, out_bytes, &docs);
}

int pfac_replace_documents_d2h(pfac_ctx *ctx, int slot, uint64_t *host_out_offsets) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.rpd_off, "pfac_replace_documents_d2h", "pfac_replace_documents", host_out_offsets, 0, s.rpd_off.n);
}

int pfac_replace_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.rp_out, "pfac_replace_d2h", "pfac_replace_leftmost_longest / pfac_replace_documents", host, first, n);
}

int pfac_extract_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, void *d_out,
                                  uint64_t out_cap, uint64_t *d_pick_offsets, uint64_t *out_bytes) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!out_bytes) return fail(ctx, PFAC_E_ARG, "null argument");
    *out_bytes = 0;
    const RpExtract ext{d_pick_offsets};
    return rp_run(ctx, ctx->slots[slot], "pfac_extract_leftmost_longest", d_input, d_sel, d_out, out_cap, out_bytes, nullptr, &ext);
}

int pfac_extract_d2h(pfac_ctx *ctx, int slot, void *host, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.ex_out, "pfac_extract_d2h", "pfac_extract_leftmost_longest", host, first, n);
}

int pfac_extract_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_pick_offsets) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.ex_off, "pfac_extract_offsets_d2h", "pfac_extract_leftmost_longest", host_pick_offsets, 0, s.ex_off.n);
}

// The token ids: checked whole, made aside, swapped in together; the old buffers are freed behind that (hipFree waits
// for the device), as the replacements are.
int pfac_table_set_token_ids(pfac_ctx *ctx, const int32_t *state_ids, uint64_t n_states, const int32_t *byte_ids) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    const std::string fn = "pfac_table_set_token_ids";
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!state_ids && n_states))
        return fail(ctx, PFAC_E_ARG, fn + ": need num_final state ids (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    for (uint64_t i = 0; i < n_states; i++)
        if (state_ids[i] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of final state " + std::to_string(i) + " is neither >= 0 nor PFAC_TOKEN_DROP");
    int32_t bytes[256];
    for (int b = 0; b < 256; b++) {
        bytes[b] = byte_ids ? byte_ids[b] : PFAC_TOKEN_DROP;
        if (bytes[b] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of byte " + std::to_string(b) + " is neither >= 0 nor PFAC_TOKEN_DROP");
    }
    USE_DEVICE(ctx);
    DevBuf<int> tok, btok;
    const uint64_t n = std::max<uint64_t>(n_states, 1);
    int rc = tok.ensure(ctx, nullptr, n, n);
    if (!rc) rc = btok.ensure(ctx, nullptr, 256, 256);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(tok.p, 0xff, n * 4));
    if (n_states) HIP_TRY(ctx, hipMemcpy(tok.p, state_ids, n_states * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(btok.p, bytes, sizeof bytes, hipMemcpyHostToDevice));
    ctx->tok = std::move(tok);                              // (a swap: the old buffers go with the two locals)
    ctx->btok = std::move(btok);
    return PFAC_OK;
}

// The documents of pfac_tokenize_documents as the caller passed them (NULL: the slot's offsets / doc_first of the
// selection, the slot-owned token offsets); tk_run without them is pfac_tokenize_leftmost_longest.
struct TkDocs {
    const uint64_t *off, *first;
    uint64_t *tok_off;
};

static int tk_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                  int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens, const TkDocs *docs) {
    s.tk_ids.invalidate();
    s.tk_pos.invalidate();
    s.tk_off.invalidate();
    s.ug_gen = 0;
    s.bpe_gen = 0;
    if (!s.scanned || !s.ll_out.done || s.ll_seq != s.scan_seq || (docs && !s.ll_docs))
        return fail(ctx, PFAC_E_STATE, fn + (docs ? " needs a pfac_records_leftmost_longest_documents since the slot's last scan"
                                                  : " needs a pfac_records_leftmost_longest since the slot's last scan"));
    if (!ctx->have_table || s.last_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
    if (!ctx->tok.p) return fail(ctx, PFAC_E_STATE, fn + ": no token ids for the uploaded table (pfac_table_set_token_ids)");
    if (!ctx->flen.p) return fail(ctx, PFAC_E_STATE, fn + ": no final-state lengths for the uploaded table");
    const pfac_record *sel;
    int rc = s.ll_out.consume(ctx, fn, "selection (d_sel)", d_sel, ANY_N, &sel);
    if (rc) return rc;
    const bool want_pos = flags & PFAC_TOKENS_POSITIONS;
    if (flags & ~PFAC_TOKENS_POSITIONS) return fail(ctx, PFAC_E_ARG, fn + ": unknown flags");
    if (d_pos && !want_pos) return fail(ctx, PFAC_E_ARG, fn + ": d_pos without PFAC_TOKENS_POSITIONS");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    const uint64_t n = s.ll_out.n, n_owned = s.last_owned, n_avail = s.last_avail, entry = s.ll_entry, ex = s.ll_exit;
    if (((uintptr_t)d_ids & 15) || ((uintptr_t)d_pos & 15) || ((uintptr_t)in & 15) || ((uintptr_t)d_sel & 7))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_input, d_ids and d_pos 16 B, d_sel 8 B)");
    if (n_owned > entry && !in) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    if (!d_input && n_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
    const unsigned long long *doff = nullptr, *dfirst = nullptr;
    unsigned long long *dtok_off = nullptr;
    if (docs) {
        doff = reinterpret_cast<const unsigned long long *>(docs->off);
        dtok_off = reinterpret_cast<unsigned long long *>(docs->tok_off);
        if (!doff) {
            if (!s.lld_own_off) return fail(ctx, PFAC_E_STATE, fn + ": the selection cut the caller's document offsets; pass them as d_doc_offsets");
            if (s.lld_gen != s.doc_gen || !s.doc.done) return fail(ctx, PFAC_E_STATE, fn + ": the slot's document offsets changed since the selection");
            doff = s.doc.buf.p;
        }
        rc = s.lld_first.consume(ctx, fn, "doc_first of the selection (d_doc_first)", docs->first, ANY_N, &dfirst);
        if (rc) return rc;
        if (((uintptr_t)doff & 7) || ((uintptr_t)dfirst & 7) || ((uintptr_t)dtok_off & 7))
            return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    }
    USE_DEVICE(ctx);
    const uint64_t n_tiles = (n_owned + WTILE - 1) / WTILE, n_groups = (n_tiles + TK_GROUP - 1) / TK_GROUP;
    uint64_t nt = 0;
    if (n_tiles) {
        rc = s.tk_first.ensure(ctx, s.stream, n_tiles + 1, quarter_more(n_tiles + 1));
        if (!rc) rc = s.tk_bm.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_wpre.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_tpre.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (!rc) rc = ensure_gsum(ctx, s, (unsigned)n_groups + 2);      // group prefixes, the total, error flag, c_{n-1}
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 24, s.stream));
        hipLaunchKernelGGL(pfac_tk_first_kernel, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, s.stream, sel,
                           (unsigned long long)n, (unsigned long long)n_tiles, s.tk_first.p);
        hipLaunchKernelGGL(pfac_tk_count_kernel, dim3((unsigned)n_groups), dim3(TK_WAVES * WAVE), 0, s.stream, in,
                           (unsigned long long)n_avail, sel, (unsigned long long)n, (unsigned long long)entry,
                           (unsigned long long)n_owned, (unsigned long long)n_tiles, ctx->flen.p, ctx->tok.p, ctx->btok.p,
                           (unsigned)ctx->plan.base.num_final, s.tk_first.p, s.tk_bm.p, s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, res);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, (unsigned)n_groups);
        rc = pass_words(ctx, s, res, 3);
        if (rc) return rc;
        nt = host_u64(s, H_PASS);
        const uint64_t err = host_u64(s, H_PASS1), c_last = host_u64(s, H_PASS2);
        if (err || (n && (c_last > n_owned ? c_last - n_owned : 0) != ex))
            return fail(ctx, PFAC_E_ARG, fn + ": the selection is not one of this scan and table");
    } else if (n) {
        return fail(ctx, PFAC_E_ARG, fn + ": the selection is not one of this scan and table");
    }
    *n_tokens = nt;
    if ((d_ids || d_pos) && nt > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(nt) + " tokens, out_cap is " + std::to_string(out_cap));
    const uint64_t n_docs = docs ? s.lld_first.n - 1 : 0;
    const uint64_t cap = align_up(nt + nt / 8, 1024);
    int *ids = nullptr;
    unsigned *pos = nullptr;
    unsigned long long *toff = nullptr;
    rc = s.tk_ids.bind(ctx, s.stream, d_ids, nt, cap, &ids);       // (everything allocated before the first write)
    if (!rc && want_pos) rc = s.tk_pos.bind(ctx, s.stream, d_pos, nt, cap, &pos);
    if (!rc && docs) rc = s.tk_off.bind(ctx, s.stream, dtok_off, n_docs + 1, docs_cap(n_docs), &toff);
    if (rc) return rc;
    if (nt) {
        if (want_pos)
            hipLaunchKernelGGL(pfac_tk_write_kernel<true>, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, in,
                               (unsigned long long)n_avail, sel, (unsigned)ctx->plan.base.num_final, ctx->tok.p, ctx->btok.p,
                               s.tk_first.p, s.tk_bm.p, s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, ids, pos);
        else
            hipLaunchKernelGGL(pfac_tk_write_kernel<false>, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, in,
                               (unsigned long long)n_avail, sel, (unsigned)ctx->plan.base.num_final, ctx->tok.p, ctx->btok.p,
                               s.tk_first.p, s.tk_bm.p, s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, ids, pos);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (docs) {
        if (n_tiles) {
            const unsigned oblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 1 + 255) / 256, 65536));
            hipLaunchKernelGGL(pfac_tk_doc_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, (unsigned long long)n_tiles, (unsigned)n_groups, s.tk_bm.p,
                               s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, toff);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemsetAsync(toff, 0, (n_docs + 1) * 8, s.stream));
        }
        s.tk_off.commit(n_docs + 1, !dtok_off);
    }
    if (want_pos) s.tk_pos.commit(nt, !d_pos);
    s.tk_ids.commit(nt, !d_ids);
    return PFAC_OK;
}

int pfac_tokenize_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                                   int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    return tk_run(ctx, ctx->slots[slot], "pfac_tokenize_leftmost_longest", d_input, d_sel, flags, d_ids, out_cap, d_pos, n_tokens, nullptr);
}

int pfac_tokenize_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                            const uint64_t *d_doc_first, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                            uint64_t *d_tok_offsets, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    const TkDocs docs{d_doc_offsets, d_doc_first, d_tok_offsets};
    return tk_run(ctx, ctx->slots[slot], "pfac_tokenize_documents", d_input, d_sel, flags, d_ids, out_cap, d_pos, n_tokens, &docs);
}

int pfac_tokens_d2h(pfac_ctx *ctx, int slot, int32_t *host_ids, uint32_t *host_pos, uint64_t first, uint64_t n) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const char *fn = "pfac_tokens_d2h", *pass = "pfac_tokenize_leftmost_longest / pfac_tokenize_documents";
    rc = fetch(ctx, s, s.tk_ids, fn, pass, host_ids, first, n);
    if (rc || !host_pos) return rc;
    return fetch(ctx, s, s.tk_pos, fn, "tokenize pass with PFAC_TOKENS_POSITIONS", host_pos, first, n);
}

int pfac_tokens_offsets_d2h(pfac_ctx *ctx, int slot, uint64_t *host_tok_off) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    return fetch(ctx, s, s.tk_off, "pfac_tokens_offsets_d2h", "pfac_tokenize_documents", host_tok_off, 0, s.tk_off.n);
}

// The WordPiece attachment: checked whole, made aside, swapped in together, as the token ids are; it leaves them alone.
int pfac_table_set_wordpiece(pfac_ctx *ctx, const int32_t *first_ids, const int32_t *cont_ids, uint64_t n_states,
                             const int32_t *byte_ids, int32_t unk_id, const uint64_t word_set[4], uint32_t max_word_bytes) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    const std::string fn = "pfac_table_set_wordpiece";
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || ((!first_ids || !cont_ids) && n_states))
        return fail(ctx, PFAC_E_ARG, fn + ": need num_final first and continuation ids (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    std::vector<int2> pairs(std::max<uint64_t>(n_states, 1), make_int2(PFAC_TOKEN_DROP, PFAC_TOKEN_DROP));
    for (uint64_t i = 0; i < n_states; i++) {
        if (first_ids[i] < PFAC_TOKEN_DROP || cont_ids[i] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": an id of final state " + std::to_string(i) + " is neither >= 0 nor PFAC_TOKEN_DROP");
        pairs[i] = make_int2(first_ids[i], cont_ids[i]);
    }
    int32_t bytes[256];
    for (int b = 0; b < 256; b++) {
        bytes[b] = byte_ids ? byte_ids[b] : PFAC_TOKEN_DROP;
        if (bytes[b] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of byte " + std::to_string(b) + " is neither >= 0 nor PFAC_TOKEN_DROP");
    }
    if (unk_id < 0) return fail(ctx, PFAC_E_ARG, fn + ": unk_id must be >= 0");
    if (max_word_bytes < 1 || max_word_bytes > 4095) return fail(ctx, PFAC_E_ARG, fn + ": max_word_bytes must lie in 1..4095");
    USE_DEVICE(ctx);
    DevBuf<int2> ids;
    DevBuf<int> btok;
    int rc = ids.ensure(ctx, nullptr, pairs.size(), pairs.size());
    if (!rc) rc = btok.ensure(ctx, nullptr, 256, 256);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ids.p, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(btok.p, bytes, sizeof bytes, hipMemcpyHostToDevice));
    ctx->wp_ids = std::move(ids);                           // (a swap: the old buffers go with the two locals)
    ctx->wp_btok = std::move(btok);
    ctx->wp_unk = unk_id;
    ctx->wp_max = max_word_bytes;
    for (int k = 0; k < 4; k++)                              // NULL: [0-9A-Za-z_]
        ctx->wp_ws.w[k] = word_set ? word_set[k] : (k == 0 ? 0x03FF000000000000ull : (k == 1 ? 0x07FFFFFE87FFFFFEull : 0ull));
    ctx->wp_gen++;
    return PFAC_OK;
}

int pfac_records_filter_roles(pfac_ctx *ctx, int slot, const void *d_input, void *d_records, uint64_t *n_kept) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_kept) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_kept = 0;
    Slot &s = ctx->slots[slot];
    const std::string fn = "pfac_records_filter_roles";
    rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    if (!ctx->wp_ids.p) return fail(ctx, PFAC_E_STATE, fn + ": no WordPiece ids for the uploaded table (pfac_table_set_wordpiece)");
    rc = last_scan_usable(ctx, s, fn, SCAN_FITS);
    if (rc) return rc;
    void *heap = d_records ? d_records : (void *)s.records.p;
    if (heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    if ((uintptr_t)in & 15) return fail(ctx, PFAC_E_ARG, fn + ": d_input must be 16-byte aligned");
    if (!d_input && s.last_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
    if (!in && s.last_total) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    USE_DEVICE(ctx);
    const uint64_t n_tiles = s.last_tiles;
    const unsigned n_groups = (unsigned)((n_tiles + XGROUP - 1) / XGROUP);
    rc = ensure_gsum(ctx, s, 1);                            // the kept total
    if (rc) return rc;
    unsigned long long *res = s.gsum.p;
    HIP_TRY(ctx, hipMemsetAsync(res, 0, 8, s.stream));
    if (n_groups) {
        auto fk = by_width(s.last_rec_bytes, [](auto w) { return pfac_filter_roles_kernel<w()>; });
        hipLaunchKernelGGL(fk, dim3((n_groups + 3) / 4), dim3(256), 0, s.stream, heap, s.tile_index.p, (unsigned long long)n_tiles,
                           (unsigned long long)s.last_cap, in, (unsigned long long)s.last_avail, (const int2 *)ctx->wp_ids.p,
                           (unsigned)ctx->plan.base.num_final, ctx->wp_ws, res);
    }
    rc = pass_words(ctx, s, res, 1);
    if (rc) return rc;
    // as after the whole-word filter: the kept records ARE the scan's records from here on
    const uint64_t total = host_u64(s, H_PASS);
    s.last_total = total;
    s.h_ctl[H_MATCHES] = (unsigned)total;
    s.h_ctl[H_MATCHES + 1] = (unsigned)(total >> 32);
    s.scan_seq++;
    s.rf_done = true;
    s.rf_gen = ctx->wp_gen;
    *n_kept = total;
    return PFAC_OK;
}

// tk_run's sibling: the same ladder and outputs, the WordPiece kernels between them
static int wp_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                  int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens, const TkDocs *docs) {
    s.tk_ids.invalidate();
    s.tk_pos.invalidate();
    s.tk_off.invalidate();
    s.ug_gen = 0;
    s.bpe_gen = 0;
    if (!s.scanned || !s.ll_out.done || s.ll_seq != s.scan_seq || (docs && !s.ll_docs))
        return fail(ctx, PFAC_E_STATE, fn + (docs ? " needs a pfac_records_leftmost_longest_documents since the slot's last scan"
                                                  : " needs a pfac_records_leftmost_longest since the slot's last scan"));
    if (!ctx->have_table || s.last_table != ctx->table_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the selection was made with an earlier table");
    if (!ctx->wp_ids.p) return fail(ctx, PFAC_E_STATE, fn + ": no WordPiece ids for the uploaded table (pfac_table_set_wordpiece)");
    if (!ctx->flen.p) return fail(ctx, PFAC_E_STATE, fn + ": no final-state lengths for the uploaded table");
    if (!s.rf_done || s.rf_gen != ctx->wp_gen)
        return fail(ctx, PFAC_E_STATE, fn + ": the scan has not been through pfac_records_filter_roles under the current WordPiece ids");
    if (s.ll_entry != 0) return fail(ctx, PFAC_E_STATE, fn + ": the selection was made from an entry other than 0 (chained ranges are out of scope)");
    const pfac_record *sel;
    int rc = s.ll_out.consume(ctx, fn, "selection (d_sel)", d_sel, ANY_N, &sel);
    if (rc) return rc;
    const bool want_pos = flags & PFAC_TOKENS_POSITIONS;
    if (flags & ~PFAC_TOKENS_POSITIONS) return fail(ctx, PFAC_E_ARG, fn + ": unknown flags");
    if (d_pos && !want_pos) return fail(ctx, PFAC_E_ARG, fn + ": d_pos without PFAC_TOKENS_POSITIONS");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    const uint64_t n = s.ll_out.n, n_owned = s.last_owned, n_avail = s.last_avail, ex = s.ll_exit;
    if (((uintptr_t)d_ids & 15) || ((uintptr_t)d_pos & 15) || ((uintptr_t)in & 15) || ((uintptr_t)d_sel & 7))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_input, d_ids and d_pos 16 B, d_sel 8 B)");
    if (n_owned && !in) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    if (!d_input && n_avail > s.input.cap) return fail(ctx, PFAC_E_ARG, fn + ": the scan read more than the slot's input buffer holds");
    const unsigned long long *doff = nullptr, *dfirst = nullptr;
    unsigned long long *dtok_off = nullptr;
    if (docs) {
        doff = reinterpret_cast<const unsigned long long *>(docs->off);
        dtok_off = reinterpret_cast<unsigned long long *>(docs->tok_off);
        if (!doff) {
            if (!s.lld_own_off) return fail(ctx, PFAC_E_STATE, fn + ": the selection cut the caller's document offsets; pass them as d_doc_offsets");
            if (s.lld_gen != s.doc_gen || !s.doc.done) return fail(ctx, PFAC_E_STATE, fn + ": the slot's document offsets changed since the selection");
            doff = s.doc.buf.p;
        }
        rc = s.lld_first.consume(ctx, fn, "doc_first of the selection (d_doc_first)", docs->first, ANY_N, &dfirst);
        if (rc) return rc;
        if (((uintptr_t)doff & 7) || ((uintptr_t)dfirst & 7) || ((uintptr_t)dtok_off & 7))
            return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    }
    USE_DEVICE(ctx);
    const uint64_t n_docs = docs ? s.lld_first.n - 1 : 0;
    const uint64_t n_tiles = (n_owned + WTILE - 1) / WTILE, n_groups = (n_tiles + TK_GROUP - 1) / TK_GROUP;
    const unsigned oblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 1 + 255) / 256, 65536));
    uint64_t nt = 0;
    if (n_tiles) {
        rc = s.tk_first.ensure(ctx, s.stream, n_tiles + 1, quarter_more(n_tiles + 1));
        if (!rc) rc = s.tk_bm.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_wpre.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_tpre.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (!rc) rc = s.wp_maps.ensure(ctx, s.stream, n_tiles * WP_MAPS * TK_WORDS, quarter_more(n_tiles) * WP_MAPS * TK_WORDS);
        if (!rc) rc = s.wp_sum.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (!rc) rc = s.wp_unk.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = ensure_gsum(ctx, s, (unsigned)n_groups + 2);      // group prefixes, the total, error flags, c_{n-1}
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 24, s.stream));
        hipLaunchKernelGGL(pfac_tk_first_kernel, dim3((unsigned)((n_tiles + 1 + 255) / 256)), dim3(256), 0, s.stream, sel,
                           (unsigned long long)n, (unsigned long long)n_tiles, s.tk_first.p);
        hipLaunchKernelGGL(pfac_wp_edge_kernel, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, in, (unsigned long long)n_avail, sel,
                           (unsigned long long)n, (unsigned long long)n_owned, ctx->flen.p, (const int2 *)ctx->wp_ids.p,
                           (const int *)ctx->wp_btok.p, (unsigned)ctx->plan.base.num_final, (const unsigned long long *)s.tk_first.p,
                           ctx->wp_ws, s.wp_maps.p, s.wp_sum.p, res);
        hipLaunchKernelGGL(pfac_wp_count_kernel, dim3((unsigned)n_groups), dim3(TK_WAVES * WAVE), 0, s.stream,
                           (const unsigned long long *)s.wp_maps.p, (const unsigned long long *)s.wp_sum.p, (unsigned long long)n_tiles,
                           ctx->wp_max, s.tk_bm.p, s.wp_unk.p, s.tk_wpre.p, s.tk_tpre.p, s.gsum.p);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, (unsigned)n_groups);
        if (docs)
            hipLaunchKernelGGL(pfac_wp_docs_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, in, ctx->wp_ws, res + 1);
        rc = pass_words(ctx, s, res, 3);
        if (rc) return rc;
        nt = host_u64(s, H_PASS);
        const uint64_t err = host_u64(s, H_PASS1), c_last = host_u64(s, H_PASS2);
        if ((err & 1) || (n && (c_last > n_owned ? c_last - n_owned : 0) != ex))
            return fail(ctx, PFAC_E_ARG, fn + ": the selection is not one of this scan and table");
        if (err & 2) return fail(ctx, PFAC_E_ARG, fn + ": a document offset lies inside a word");
    } else if (n) {
        return fail(ctx, PFAC_E_ARG, fn + ": the selection is not one of this scan and table");
    }
    *n_tokens = nt;
    if ((d_ids || d_pos) && nt > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(nt) + " tokens, out_cap is " + std::to_string(out_cap));
    const uint64_t cap = align_up(nt + nt / 8, 1024);
    int *ids = nullptr;
    unsigned *pos = nullptr;
    unsigned long long *toff = nullptr;
    rc = s.tk_ids.bind(ctx, s.stream, d_ids, nt, cap, &ids);       // (everything allocated before the first write)
    if (!rc && want_pos) rc = s.tk_pos.bind(ctx, s.stream, d_pos, nt, cap, &pos);
    if (!rc && docs) rc = s.tk_off.bind(ctx, s.stream, dtok_off, n_docs + 1, docs_cap(n_docs), &toff);
    if (rc) return rc;
    if (nt) {
        auto wk = want_pos ? pfac_wp_write_kernel<true> : pfac_wp_write_kernel<false>;
        hipLaunchKernelGGL(wk, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, in, (unsigned long long)n_avail, sel,
                           (unsigned)ctx->plan.base.num_final, (const int2 *)ctx->wp_ids.p, (const int *)ctx->wp_btok.p, ctx->wp_unk,
                           ctx->wp_ws, (const unsigned long long *)s.tk_first.p, (const unsigned long long *)s.wp_maps.p,
                           (const unsigned long long *)s.tk_bm.p, (const unsigned long long *)s.wp_unk.p,
                           (const unsigned short *)s.tk_wpre.p, (const unsigned *)s.tk_tpre.p, (const unsigned long long *)s.gsum.p,
                           ids, pos);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (docs) {
        if (n_tiles) {
            hipLaunchKernelGGL(pfac_tk_doc_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, (unsigned long long)n_tiles, (unsigned)n_groups, s.tk_bm.p,
                               s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, toff);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemsetAsync(toff, 0, (n_docs + 1) * 8, s.stream));
        }
        s.tk_off.commit(n_docs + 1, !dtok_off);
    }
    if (want_pos) s.tk_pos.commit(nt, !d_pos);
    s.tk_ids.commit(nt, !d_ids);
    return PFAC_OK;
}

int pfac_wordpiece_leftmost_longest(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, uint32_t flags,
                                    int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    return wp_run(ctx, ctx->slots[slot], "pfac_wordpiece_leftmost_longest", d_input, d_sel, flags, d_ids, out_cap, d_pos, n_tokens, nullptr);
}

int pfac_wordpiece_documents(pfac_ctx *ctx, int slot, const void *d_input, const pfac_record *d_sel, const uint64_t *d_doc_offsets,
                             const uint64_t *d_doc_first, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                             uint64_t *d_tok_offsets, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    const TkDocs docs{d_doc_offsets, d_doc_first, d_tok_offsets};
    return wp_run(ctx, ctx->slots[slot], "pfac_wordpiece_documents", d_input, d_sel, flags, d_ids, out_cap, d_pos, n_tokens, &docs);
}

// The Unigram attachment: checked whole, made aside, swapped in together, as the WordPiece one is; it leaves that one
// and the token ids alone.
int pfac_table_set_unigram(pfac_ctx *ctx, const pfac_unigram_piece *pieces, uint64_t n_states, const int32_t *byte_ids,
                           int32_t byte_score, int32_t unk_id, const uint64_t word_set[4], uint32_t max_word_bytes) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    const std::string fn = "pfac_table_set_unigram";
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!pieces && n_states))
        return fail(ctx, PFAC_E_ARG, fn + ": need num_final pieces (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    if (max_word_bytes < 1 || max_word_bytes > 4095) return fail(ctx, PFAC_E_ARG, fn + ": max_word_bytes must lie in 1..4095");
    // sums stay in int32: a path has at most max_word_bytes edges (and one more for slack)
    const auto fits = [&](int32_t sc) { return (uint64_t)std::llabs((long long)sc) * (max_word_bytes + 1ull) < (1ull << 31); };
    std::vector<int4> quads(std::max<uint64_t>(n_states, 1), make_int4(PFAC_TOKEN_DROP, PFAC_TOKEN_DROP, 0, 0));
    for (uint64_t i = 0; i < n_states; i++) {
        const pfac_unigram_piece &p = pieces[i];
        if (p.first_id < PFAC_TOKEN_DROP || p.cont_id < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": an id of final state " + std::to_string(i) + " is neither >= 0 nor PFAC_TOKEN_DROP");
        if (!fits(p.first_score) || !fits(p.cont_score))
            return fail(ctx, PFAC_E_ARG, fn + ": a score of final state " + std::to_string(i) + " times max_word_bytes + 1 does not fit int32");
        quads[i] = make_int4(p.first_id, p.cont_id, p.first_score, p.cont_score);
    }
    int32_t bytes[256];
    for (int b = 0; b < 256; b++) {
        bytes[b] = byte_ids ? byte_ids[b] : PFAC_TOKEN_DROP;
        if (bytes[b] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of byte " + std::to_string(b) + " is neither >= 0 nor PFAC_TOKEN_DROP");
    }
    if (!fits(byte_score)) return fail(ctx, PFAC_E_ARG, fn + ": byte_score times max_word_bytes + 1 does not fit int32");
    if (unk_id < PFAC_TOKEN_DROP) return fail(ctx, PFAC_E_ARG, fn + ": unk_id must be >= 0 or PFAC_TOKEN_DROP");
    USE_DEVICE(ctx);
    DevBuf<int4> dp;
    DevBuf<int> btok;
    int rc = dp.ensure(ctx, nullptr, quads.size(), quads.size());
    if (!rc) rc = btok.ensure(ctx, nullptr, 256, 256);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(dp.p, quads.data(), quads.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(btok.p, bytes, sizeof bytes, hipMemcpyHostToDevice));
    ctx->ug_pieces = std::move(dp);                         // (a swap: the old buffers go with the two locals)
    ctx->ug_btok = std::move(btok);
    ctx->ug_unk = unk_id;
    ctx->ug_bscore = byte_score;
    ctx->ug_max = max_word_bytes;
    for (int k = 0; k < 4; k++)                              // NULL: everything but \t \n \v \f \r and space
        ctx->ug_ws.w[k] = word_set ? word_set[k] : (k == 0 ? ~0x0000000100003E00ull : ~0ull);
    ctx->ug_gen++;
    for (auto &sl : ctx->slots) {                            // a slot-owned result of the earlier attachment is stale
        if (!sl.ug_gen) continue;
        sl.tk_ids.invalidate();
        sl.tk_pos.invalidate();
        sl.tk_off.invalidate();
        sl.ug_gen = 0;
    }
    return PFAC_OK;
}

struct UgDocs {
    const uint64_t *off;
    uint64_t n_docs;
    uint64_t *tok_off;
};

// wp_run's sibling over the record heap: the filters' ladder, the tokenizer's outputs, the Unigram kernels between them
static int ug_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_input, const void *d_records, uint32_t flags,
                  int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens, const UgDocs *docs) {
    s.tk_ids.invalidate();
    s.tk_pos.invalidate();
    s.tk_off.invalidate();
    s.ug_gen = 0;
    s.bpe_gen = 0;
    int rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    if (!ctx->ug_pieces.p) return fail(ctx, PFAC_E_STATE, fn + ": no Unigram pieces for the uploaded table (pfac_table_set_unigram)");
    if (s.last_used > s.last_cap) return fail(ctx, PFAC_E_STATE, fn + ": the slot's last scan overflowed its record heap: scan again with a larger one");
    if (!d_records && (const void *)s.records.p != s.last_records)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's record heap was replaced since its last scan");
    if (!d_input && s.last_avail > s.input.cap)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's input buffer was replaced since its last scan");
    const bool want_pos = flags & PFAC_TOKENS_POSITIONS;
    if (flags & ~PFAC_TOKENS_POSITIONS) return fail(ctx, PFAC_E_ARG, fn + ": unknown flags");
    if (d_pos && !want_pos) return fail(ctx, PFAC_E_ARG, fn + ": d_pos without PFAC_TOKENS_POSITIONS");
    const void *heap = d_records ? d_records : (const void *)s.records.p;
    if (heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    const uint64_t n_owned = s.last_owned, n_avail = s.last_avail;
    if (((uintptr_t)d_ids & 15) || ((uintptr_t)d_pos & 15) || ((uintptr_t)in & 15))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_input, d_ids and d_pos 16 B)");
    if (n_owned && !in) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    const unsigned long long *doff = nullptr;
    unsigned long long *dtok_off = nullptr;
    uint64_t n_docs = 0;
    if (docs) {
        n_docs = docs->n_docs;
        dtok_off = reinterpret_cast<unsigned long long *>(docs->tok_off);
        rc = resolve_docs(ctx, s, fn, docs->off, n_docs, (uintptr_t)dtok_off, &doff);
        if (rc) return rc;
        if (((uintptr_t)doff & 7) || ((uintptr_t)dtok_off & 7)) return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    }
    USE_DEVICE(ctx);
    const uint64_t n_tiles = (n_owned + WTILE - 1) / WTILE, n_groups = (n_tiles + TK_GROUP - 1) / TK_GROUP;
    const unsigned oblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 1 + 255) / 256, 65536));
    const int rb = s.last_rec_bytes;
    const bool wide = ctx->ug_max > 255;                     // the region's overhang: 256 bytes, or a whole tile
    uint64_t nt = 0;
    if (n_tiles) {
        rc = s.tk_bm.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_wpre.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_tpre.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (!rc) rc = s.ug_maps.ensure(ctx, s.stream, n_tiles * UG_MAPS * TK_WORDS, quarter_more(n_tiles) * UG_MAPS * TK_WORDS);
        if (!rc) rc = ensure_gsum(ctx, s, (unsigned)n_groups + 1);      // group prefixes, the total, error flags
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        auto sk = by_width(rb, [wide](auto w) { return wide ? pfac_ug_solve_kernel<w(), WTILE> : pfac_ug_solve_kernel<w(), 256>; });
        hipLaunchKernelGGL(sk, dim3((unsigned)n_tiles), dim3(UG_THREADS), 0, s.stream, heap, (const unsigned long long *)s.tile_index.p,
                           (unsigned long long)s.last_tiles, (unsigned long long)s.last_cap, in, (unsigned long long)n_avail,
                           (unsigned long long)n_owned, ctx->flen.p, (const int4 *)ctx->ug_pieces.p, (const int *)ctx->ug_btok.p,
                           (unsigned)ctx->plan.base.num_final, ctx->ug_bscore, ctx->ug_unk, ctx->ug_max, ctx->ug_ws, s.ug_maps.p,
                           s.tk_bm.p, s.tk_wpre.p, s.tk_tpre.p);
        hipLaunchKernelGGL(pfac_ug_group_kernel, dim3((unsigned)n_groups), dim3(WAVE), 0, s.stream, s.tk_tpre.p,
                           (unsigned long long)n_tiles, s.gsum.p);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, (unsigned)n_groups);
        if (docs) {
            hipLaunchKernelGGL(pfac_offsets_check_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, res + 1);
            hipLaunchKernelGGL(pfac_wp_docs_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, in, ctx->ug_ws, res + 1);
        }
        rc = pass_words(ctx, s, res, 2);
        if (rc) return rc;
        nt = host_u64(s, H_PASS);
        if (host_u64(s, H_PASS1) & 1) return bad_doc_offsets(ctx, s, fn);
        if (host_u64(s, H_PASS1) & 2) return fail(ctx, PFAC_E_ARG, fn + ": a document offset lies inside a word");
    } else if (docs) {                                       // nothing owned: the offsets rule alone (every offset is 0)
        rc = ensure_gsum(ctx, s, 1);
        if (rc) return rc;
        unsigned long long *res = s.gsum.p;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        hipLaunchKernelGGL(pfac_offsets_check_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                           (unsigned long long)n_owned, res + 1);
        rc = pass_words(ctx, s, res, 2);
        if (rc) return rc;
        if (host_u64(s, H_PASS1) & 1) return bad_doc_offsets(ctx, s, fn);
    }
    *n_tokens = nt;
    if ((d_ids || d_pos) && nt > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(nt) + " tokens, out_cap is " + std::to_string(out_cap));
    const uint64_t cap = align_up(nt + nt / 8, 1024);
    int *ids = nullptr;
    unsigned *pos = nullptr;
    unsigned long long *toff = nullptr;
    rc = s.tk_ids.bind(ctx, s.stream, d_ids, nt, cap, &ids);       // (everything allocated before the first write)
    if (!rc && want_pos) rc = s.tk_pos.bind(ctx, s.stream, d_pos, nt, cap, &pos);
    if (!rc && docs) rc = s.tk_off.bind(ctx, s.stream, dtok_off, n_docs + 1, docs_cap(n_docs), &toff);
    if (rc) return rc;
    if (nt) {
        auto wk = by_width(rb, [want_pos](auto w) { return want_pos ? pfac_ug_write_kernel<w(), true> : pfac_ug_write_kernel<w(), false>; });
        hipLaunchKernelGGL(wk, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, heap, (const unsigned long long *)s.tile_index.p,
                           (unsigned long long)s.last_tiles, (unsigned long long)s.last_cap, in, (unsigned long long)n_avail, ctx->flen.p,
                           (const int4 *)ctx->ug_pieces.p, (const int *)ctx->ug_btok.p, (unsigned)ctx->plan.base.num_final, ctx->ug_unk,
                           ctx->ug_ws, (const unsigned long long *)s.ug_maps.p, (unsigned long long)n_tiles,
                           (const unsigned long long *)s.tk_bm.p, (const unsigned short *)s.tk_wpre.p, (const unsigned *)s.tk_tpre.p,
                           (const unsigned long long *)s.gsum.p, ids, pos);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (docs) {
        if (n_tiles) {
            hipLaunchKernelGGL(pfac_tk_doc_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, (unsigned long long)n_tiles, (unsigned)n_groups, s.tk_bm.p,
                               s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, toff);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemsetAsync(toff, 0, (n_docs + 1) * 8, s.stream));
        }
        s.tk_off.commit(n_docs + 1, !dtok_off);
    }
    if (want_pos) s.tk_pos.commit(nt, !d_pos);
    s.tk_ids.commit(nt, !d_ids);
    s.ug_gen = ctx->ug_gen;
    return PFAC_OK;
}

int pfac_unigram_records(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, uint32_t flags, int32_t *d_ids,
                         uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    return ug_run(ctx, ctx->slots[slot], "pfac_unigram_records", d_input, d_records, flags, d_ids, out_cap, d_pos, n_tokens, nullptr);
}

int pfac_unigram_documents(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, const uint64_t *d_doc_offsets,
                           uint64_t n_docs, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                           uint64_t *d_tok_offsets, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    const UgDocs docs{d_doc_offsets, n_docs, d_tok_offsets};
    return ug_run(ctx, ctx->slots[slot], "pfac_unigram_documents", d_input, d_records, flags, d_ids, out_cap, d_pos, n_tokens, &docs);
}

// The BPE attachment: checked whole, made aside, swapped in together, as the Unigram one is; it leaves the other three
// attachments alone.
int pfac_table_set_bpe(pfac_ctx *ctx, const pfac_bpe_piece *pieces, uint64_t n_states, const int32_t *byte_ids,
                       const uint64_t word_set[4], int32_t lead, uint32_t max_word_bytes) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    const std::string fn = "pfac_table_set_bpe";
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, fn + " before a table upload");
    if (n_states != (uint64_t)ctx->plan.base.num_final || (!pieces && n_states))
        return fail(ctx, PFAC_E_ARG, fn + ": need num_final pieces (num_final " + std::to_string(ctx->plan.base.num_final) + ")");
    if (max_word_bytes < 1 || max_word_bytes > 255) return fail(ctx, PFAC_E_ARG, fn + ": max_word_bytes must lie in 1..255");
    std::vector<int4> quads(std::max<uint64_t>(n_states, 1), make_int4(PFAC_TOKEN_DROP, 0, 0, 0));
    for (uint64_t i = 0; i < n_states; i++) {
        const pfac_bpe_piece &p = pieces[i];
        if (p.id < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of final state " + std::to_string(i) + " is neither >= 0 nor PFAC_TOKEN_DROP");
        if (p.rank < 0) return fail(ctx, PFAC_E_ARG, fn + ": the rank of final state " + std::to_string(i) + " is negative");
        if (p.reserved) return fail(ctx, PFAC_E_ARG, fn + ": the reserved field of final state " + std::to_string(i) + " is not 0");
        quads[i] = make_int4(p.id, p.rank, (int)p.split, 0);
    }
    int32_t bytes[256];
    for (int b = 0; b < 256; b++) {
        bytes[b] = byte_ids ? byte_ids[b] : PFAC_TOKEN_DROP;
        if (bytes[b] < PFAC_TOKEN_DROP)
            return fail(ctx, PFAC_E_ARG, fn + ": the id of byte " + std::to_string(b) + " is neither >= 0 nor PFAC_TOKEN_DROP");
    }
    WordSet ws;
    for (int k = 0; k < 4; k++)                              // NULL: everything but \t \n \v \f \r and space
        ws.w[k] = word_set ? word_set[k] : (k == 0 ? ~0x0000000100003E00ull : ~0ull);
    if (lead < -1 || lead > 255) return fail(ctx, PFAC_E_ARG, fn + ": lead must be a byte value or -1");
    if (lead >= 0 && (ws.w[lead >> 6] >> (lead & 63) & 1ull)) return fail(ctx, PFAC_E_ARG, fn + ": the lead byte is a word byte");
    USE_DEVICE(ctx);
    DevBuf<int4> dp;
    DevBuf<int> btok;
    int rc = dp.ensure(ctx, nullptr, quads.size(), quads.size());
    if (!rc) rc = btok.ensure(ctx, nullptr, 256, 256);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(dp.p, quads.data(), quads.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(btok.p, bytes, sizeof bytes, hipMemcpyHostToDevice));
    ctx->bpe_pieces = std::move(dp);                        // (a swap: the old buffers go with the two locals)
    ctx->bpe_btok = std::move(btok);
    ctx->bpe_lead = lead;
    ctx->bpe_max = max_word_bytes;
    ctx->bpe_ws = ws;
    ctx->bpe_gen++;
    for (auto &sl : ctx->slots) {                            // a slot-owned result of the earlier attachment is stale
        if (!sl.bpe_gen) continue;
        sl.tk_ids.invalidate();
        sl.tk_pos.invalidate();
        sl.tk_off.invalidate();
        sl.bpe_gen = 0;
    }
    return PFAC_OK;
}

// ug_run's sibling: the same ladder, buffers and outputs, the BPE kernels between them
static int bpe_run(pfac_ctx *ctx, Slot &s, const std::string &fn, const void *d_input, const void *d_records, uint32_t flags,
                   int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens, const UgDocs *docs) {
    s.tk_ids.invalidate();
    s.tk_pos.invalidate();
    s.tk_off.invalidate();
    s.ug_gen = 0;
    s.bpe_gen = 0;
    int rc = last_scan_usable(ctx, s, fn, SCAN_FINISHED | SCAN_LENGTHS | SCAN_TABLE);
    if (rc) return rc;
    if (!ctx->bpe_pieces.p) return fail(ctx, PFAC_E_STATE, fn + ": no BPE pieces for the uploaded table (pfac_table_set_bpe)");
    if (s.last_used > s.last_cap) return fail(ctx, PFAC_E_STATE, fn + ": the slot's last scan overflowed its record heap: scan again with a larger one");
    if (!d_records && (const void *)s.records.p != s.last_records)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's record heap was replaced since its last scan");
    if (!d_input && s.last_avail > s.input.cap)
        return fail(ctx, PFAC_E_STATE, fn + ": the slot's input buffer was replaced since its last scan");
    const bool want_pos = flags & PFAC_TOKENS_POSITIONS;
    if (flags & ~PFAC_TOKENS_POSITIONS) return fail(ctx, PFAC_E_ARG, fn + ": unknown flags");
    if (d_pos && !want_pos) return fail(ctx, PFAC_E_ARG, fn + ": d_pos without PFAC_TOKENS_POSITIONS");
    const void *heap = d_records ? d_records : (const void *)s.records.p;
    if (heap != s.last_records) return fail(ctx, PFAC_E_ARG, fn + ": d_records is not the record heap of the slot's last scan");
    const unsigned char *in = d_input ? static_cast<const unsigned char *>(d_input) : s.input.p;
    const uint64_t n_owned = s.last_owned, n_avail = s.last_avail;
    if (((uintptr_t)d_ids & 15) || ((uintptr_t)d_pos & 15) || ((uintptr_t)in & 15))
        return fail(ctx, PFAC_E_ARG, fn + ": misaligned buffer (d_input, d_ids and d_pos 16 B)");
    if (n_owned && !in) return fail(ctx, PFAC_E_ARG, fn + ": no input buffer");
    const unsigned long long *doff = nullptr;
    unsigned long long *dtok_off = nullptr;
    uint64_t n_docs = 0;
    if (docs) {
        n_docs = docs->n_docs;
        dtok_off = reinterpret_cast<unsigned long long *>(docs->tok_off);
        rc = resolve_docs(ctx, s, fn, docs->off, n_docs, (uintptr_t)dtok_off, &doff);
        if (rc) return rc;
        if (((uintptr_t)doff & 7) || ((uintptr_t)dtok_off & 7)) return fail(ctx, PFAC_E_ARG, fn + ": device buffers must be 8-byte aligned");
    }
    USE_DEVICE(ctx);
    const uint64_t n_tiles = (n_owned + WTILE - 1) / WTILE, n_groups = (n_tiles + TK_GROUP - 1) / TK_GROUP;
    const unsigned oblocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_docs + 1 + 255) / 256, 65536));
    const int rb = s.last_rec_bytes;
    uint64_t nt = 0;
    if (n_tiles) {
        rc = s.tk_bm.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_wpre.ensure(ctx, s.stream, n_tiles * TK_WORDS, quarter_more(n_tiles) * TK_WORDS);
        if (!rc) rc = s.tk_tpre.ensure(ctx, s.stream, n_tiles, quarter_more(n_tiles));
        if (!rc) rc = s.bpe_maps.ensure(ctx, s.stream, n_tiles * BPE_MAPS * TK_WORDS, quarter_more(n_tiles) * BPE_MAPS * TK_WORDS);
        if (!rc) rc = ensure_gsum(ctx, s, (unsigned)n_groups + 1);      // group prefixes, the total, error flags
        if (rc) return rc;
        unsigned long long *res = s.gsum.p + n_groups;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        auto sk = by_width(rb, [](auto w) { return pfac_bpe_solve_kernel<w()>; });
        hipLaunchKernelGGL(sk, dim3((unsigned)n_tiles), dim3(BPE_THREADS), 0, s.stream, heap, (const unsigned long long *)s.tile_index.p,
                           (unsigned long long)s.last_tiles, (unsigned long long)s.last_cap, in, (unsigned long long)n_avail,
                           (unsigned long long)n_owned, ctx->flen.p, (const int4 *)ctx->bpe_pieces.p, (const int *)ctx->bpe_btok.p,
                           (unsigned)ctx->plan.base.num_final, ctx->bpe_lead, ctx->bpe_max, ctx->bpe_ws, s.bpe_maps.p, s.tk_bm.p,
                           s.tk_wpre.p, s.tk_tpre.p);
        hipLaunchKernelGGL(pfac_ug_group_kernel, dim3((unsigned)n_groups), dim3(WAVE), 0, s.stream, s.tk_tpre.p,
                           (unsigned long long)n_tiles, s.gsum.p);
        hipLaunchKernelGGL(pfac_scan_groups_kernel, dim3(1), dim3(1024), 0, s.stream, s.gsum.p, (unsigned)n_groups);
        if (docs) {
            hipLaunchKernelGGL(pfac_offsets_check_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, res + 1);
            hipLaunchKernelGGL(pfac_bpe_docs_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, in, ctx->bpe_ws, ctx->bpe_lead, res + 1);
        }
        rc = pass_words(ctx, s, res, 2);
        if (rc) return rc;
        nt = host_u64(s, H_PASS);
        if (host_u64(s, H_PASS1) & 1) return bad_doc_offsets(ctx, s, fn);
        if (host_u64(s, H_PASS1) & 2) return fail(ctx, PFAC_E_ARG, fn + ": a document offset lies inside a word");
    } else if (docs) {                                       // nothing owned: the offsets rule alone (every offset is 0)
        rc = ensure_gsum(ctx, s, 1);
        if (rc) return rc;
        unsigned long long *res = s.gsum.p;
        HIP_TRY(ctx, hipMemsetAsync(res, 0, 16, s.stream));
        hipLaunchKernelGGL(pfac_offsets_check_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                           (unsigned long long)n_owned, res + 1);
        rc = pass_words(ctx, s, res, 2);
        if (rc) return rc;
        if (host_u64(s, H_PASS1) & 1) return bad_doc_offsets(ctx, s, fn);
    }
    *n_tokens = nt;
    if ((d_ids || d_pos) && nt > out_cap)
        return fail(ctx, PFAC_E_OVERFLOW, fn + ": " + std::to_string(nt) + " tokens, out_cap is " + std::to_string(out_cap));
    const uint64_t cap = align_up(nt + nt / 8, 1024);
    int *ids = nullptr;
    unsigned *pos = nullptr;
    unsigned long long *toff = nullptr;
    rc = s.tk_ids.bind(ctx, s.stream, d_ids, nt, cap, &ids);       // (everything allocated before the first write)
    if (!rc && want_pos) rc = s.tk_pos.bind(ctx, s.stream, d_pos, nt, cap, &pos);
    if (!rc && docs) rc = s.tk_off.bind(ctx, s.stream, dtok_off, n_docs + 1, docs_cap(n_docs), &toff);
    if (rc) return rc;
    if (nt) {
        auto wk = by_width(rb, [want_pos](auto w) { return want_pos ? pfac_bpe_write_kernel<w(), true> : pfac_bpe_write_kernel<w(), false>; });
        hipLaunchKernelGGL(wk, dim3((unsigned)n_tiles), dim3(WAVE), 0, s.stream, heap, (const unsigned long long *)s.tile_index.p,
                           (unsigned long long)s.last_tiles, (unsigned long long)s.last_cap, in, (unsigned long long)n_avail, ctx->flen.p,
                           (const int4 *)ctx->bpe_pieces.p, (const int *)ctx->bpe_btok.p, (unsigned)ctx->plan.base.num_final,
                           (const unsigned long long *)s.bpe_maps.p, (unsigned long long)n_tiles, (const unsigned long long *)s.tk_bm.p,
                           (const unsigned short *)s.tk_wpre.p, (const unsigned *)s.tk_tpre.p, (const unsigned long long *)s.gsum.p, ids, pos);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (docs) {
        if (n_tiles) {
            hipLaunchKernelGGL(pfac_tk_doc_kernel, dim3(oblocks), dim3(256), 0, s.stream, doff, (unsigned long long)n_docs,
                               (unsigned long long)n_owned, (unsigned long long)n_tiles, (unsigned)n_groups, s.tk_bm.p,
                               s.tk_wpre.p, s.tk_tpre.p, s.gsum.p, toff);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemsetAsync(toff, 0, (n_docs + 1) * 8, s.stream));
        }
        s.tk_off.commit(n_docs + 1, !dtok_off);
    }
    if (want_pos) s.tk_pos.commit(nt, !d_pos);
    s.tk_ids.commit(nt, !d_ids);
    s.bpe_gen = ctx->bpe_gen;
    return PFAC_OK;
}

int pfac_bpe_records(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, uint32_t flags, int32_t *d_ids,
                     uint64_t out_cap, uint32_t *d_pos, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    return bpe_run(ctx, ctx->slots[slot], "pfac_bpe_records", d_input, d_records, flags, d_ids, out_cap, d_pos, n_tokens, nullptr);
}

int pfac_bpe_documents(pfac_ctx *ctx, int slot, const void *d_input, const void *d_records, const uint64_t *d_doc_offsets,
                       uint64_t n_docs, uint32_t flags, int32_t *d_ids, uint64_t out_cap, uint32_t *d_pos,
                       uint64_t *d_tok_offsets, uint64_t *n_tokens) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!n_tokens) return fail(ctx, PFAC_E_ARG, "null argument");
    *n_tokens = 0;
    const UgDocs docs{d_doc_offsets, n_docs, d_tok_offsets};
    return bpe_run(ctx, ctx->slots[slot], "pfac_bpe_documents", d_input, d_records, flags, d_ids, out_cap, d_pos, n_tokens, &docs);
}

int pfac_fill_tiled(pfac_ctx *ctx, int slot, void *d_dst, uint64_t n, const void *host_pattern, uint32_t period, uint64_t phase) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!d_dst || !host_pattern || period == 0 || ((uintptr_t)d_dst & 15)) return fail(ctx, PFAC_E_ARG, "bad argument to pfac_fill_tiled");
    Slot &s = ctx->slots[slot];
    USE_DEVICE(ctx);
    DevBuf<unsigned char> d_pat;
    rc = d_pat.ensure(ctx, nullptr, period, period);
    if (rc) return rc;
    hipError_t e = hipMemcpy(d_pat.p, host_pattern, period, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL(pfac_fill_tiled_kernel, dim3(2048), dim3(256), 0, s.stream, static_cast<unsigned char *>(d_dst),
                           (unsigned long long)n, d_pat.p, period, (unsigned long long)phase);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess) return fail(ctx, PFAC_E_HIP, std::string("pfac_fill_tiled: ") + hipGetErrorString(e));
    return PFAC_OK;
}

int pfac_fill_random(pfac_ctx *ctx, int slot, void *d_dst, uint64_t n, uint64_t seed) {
    int rc = check_slot(ctx, slot);
    if (rc) return rc;
    if (!d_dst || ((uintptr_t)d_dst & 7) || (n & 7)) return fail(ctx, PFAC_E_ARG, "pfac_fill_random: dst and n must be multiples of 8");
    Slot &s = ctx->slots[slot];
    USE_DEVICE(ctx);
    if (n) {
        hipLaunchKernelGGL(pfac_fill_random_kernel, dim3(2048), dim3(256), 0, s.stream,
                           static_cast<unsigned long long *>(d_dst), (unsigned long long)(n / 8), (unsigned long long)seed);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(s.stream));
    return PFAC_OK;
}

int pfac_scan_info(pfac_ctx *ctx, int *variant, int *tile_bytes, int *grid_blocks, int *lds_bytes) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "no table uploaded");
    if (variant) *variant = ctx->plan.variant;
    if (tile_bytes) *tile_bytes = WTILE;
    if (grid_blocks) *grid_blocks = ctx->plan.grid_blocks;
    if (lds_bytes) *lds_bytes = ctx->layout(ctx->run_dense()).lds_bytes;
    return PFAC_OK;
}

int pfac_scan_staging(pfac_ctx *ctx, int *buffers, uint32_t *records_per_buffer) {
    if (!ctx) return fail(nullptr, PFAC_E_ARG, "null context");
    if (!ctx->have_table) return fail(ctx, PFAC_E_STATE, "no table uploaded");
    const bool dense = ctx->run_dense();
    const StageLayout &L = ctx->layout(dense);
    if (buffers) *buffers = L.nbuf;
    // (dense mode's second form has no staging buffer: what bounds a tile there is the wave's record log)
    if (records_per_buffer) *records_per_buffer = dense && ctx->plan.dense2 ? ctx->plan.base.d2log_cap : L.stage_cap;
    return PFAC_OK;
}

// GPU_Malloc_Memory + GPU_TraceTable + GPU_Free_memory (master_kernel.cu:188-524), one synchronous call.
int pfac_trace_table_compat(const pfac_thread_data *d, int device) {
    if (!d || !d->input_string || !d->match_result || !d->s0Table || !d->r || !d->HT || !d->val || d->input_size < 0 ||
        d->max_pat_len < 1 || d->max_pat_len > HALO_MAX - 1)
        return fail(nullptr, PFAC_E_ARG, "bad pfac_thread_data");
    int wbit = 0;
    if (d->width < 1 || d->width > 4096 || (d->width & (d->width - 1))) return fail(nullptr, PFAC_E_ARG, "width must be a power of two <= 4096");
    while ((d->width >> wbit) != 1) wbit++;
    const int max_row = (int)(((int64_t)d->state_num * 256) / d->width) + 1;
    const int ht = d->HTSize > 0 ? d->HTSize : 1;
    std::vector<int32_t> blob((size_t)PFAC_BLOB_HEADER_WORDS + 256 + max_row + 2 * (size_t)ht + d->final_state_num, 0);
    blob[0] = PFAC_BLOB_MAGIC; blob[1] = PFAC_BLOB_VERSION; blob[2] = d->width; blob[3] = wbit;
    blob[4] = d->final_state_num; blob[5] = d->final_state_num; blob[6] = d->state_num; blob[7] = d->max_pat_len;
    blob[8] = max_row; blob[9] = ht;
    int32_t *p = blob.data() + PFAC_BLOB_HEADER_WORDS;
    memcpy(p, d->s0Table, 256 * 4); p += 256;
    memcpy(p, d->r, (size_t)max_row * 4); p += max_row;
    if (d->HTSize > 0) { memcpy(p, d->HT, (size_t)ht * 4); memcpy(p + ht, d->val, (size_t)ht * 4); }
    else { p[0] = -1; p[ht] = -1; }
    p += 2 * (size_t)ht;
    for (int i = 0; i < d->final_state_num; i++) p[i] = i;
    pfac_ctx *ctx = nullptr;
    int rc = pfac_ctx_create(device, 1, &ctx);
    if (rc) return rc;
    const uint64_t N = (uint64_t)d->input_size;
    uint64_t cap = N / 4 + 4096;
    std::vector<pfac_record> rec;
    uint64_t n = 0;
    rc = pfac_table_upload(ctx, blob.data(), blob.size());
    if (!rc) rc = pfac_slot_reserve(ctx, 0, N, cap);
    if (!rc && N) rc = pfac_slot_h2d(ctx, 0, d->input_string, N, 0);
    for (int attempt = 0; !rc && attempt < 4; attempt++) {
        rc = pfac_scan_async(ctx, 0, nullptr, N, N, nullptr, 0);
        if (!rc) rc = pfac_scan_finish(ctx, 0, &n);
        if (rc == PFAC_E_OVERFLOW && attempt < 3) {
            uint64_t hint = 0;
            rc = pfac_scan_capacity_hint(ctx, 0, &hint);
            cap = hint > 2 * cap ? hint : 2 * cap;
            if (!rc) rc = pfac_slot_reserve(ctx, 0, N, cap);
            continue;
        }
        break;
    }
    if (!rc) {
        rec.resize(n);
        rc = pfac_records_d2h(ctx, 0, nullptr, rec.data(), 0, n);
        if (!rc) rc = pfac_slot_sync(ctx, 0);
    }
    if (!rc) {
        // expand into the reference's dense layout (master_kernel.cu:104-115, memset :236)
        memset(d->match_result, 0xFF, (size_t)N * d->max_pat_len * sizeof(unsigned int));
        uint64_t k = 0;
        while (k < n) {
            uint64_t pos = rec[k].pos, j = 0;
            while (k < n && rec[k].pos == pos) {
                if (j < (uint64_t)d->max_pat_len) d->match_result[pos * d->max_pat_len + j] = rec[k].state;
                j++; k++;
            }
        }
    }
    std::string msg = ctx->err;
    pfac_ctx_destroy(ctx);
    if (rc) g_err = msg;
    return rc;
}

}  // extern "C"
