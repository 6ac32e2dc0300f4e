/*
 * pfac_fold.h -- the ASCII case fold of PFAC_FOLD_ASCII, one definition for the scan kernel (pfac_hip.hip) and the host
 * (pfac_table.c: pfac_fold_ascii, the nocase builders).  Plain C, usable from host and device code.
 *
 * Every byte 0x41..0x5A ('A'..'Z') gets 0x20 or-ed in; every other byte is unchanged.  Bytes >= 0x80 never change, so
 * UTF-8 sequences pass through whole (no Latin-1 folding).
 */
#ifndef PFAC_FOLD_H
#define PFAC_FOLD_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFAC_FOLD_FN static __host__ __device__ __forceinline__
#else
#define PFAC_FOLD_FN static inline
#endif

/* Four bytes at once, carry-free: with the top bit of every byte masked off, b + 0x3F has bit 7 set iff b >= 0x41 and
 * b + 0x25 has it set iff b >= 0x5B; neither sum exceeds 0xBE, so no carry leaves a byte.  "First and not second, and the
 * byte's own top bit clear" marks the upper-case letters in bit 7; >> 2 moves the mark to bit 5 (0x20).  Eight integer
 * operations per dword, no table. */
PFAC_FOLD_FN uint32_t pfac_fold_dword(uint32_t x) {
    const uint32_t x7 = x & 0x7F7F7F7Fu;
    const uint32_t ge_A = x7 + 0x3F3F3F3Fu;
    const uint32_t gt_Z = x7 + 0x25252525u;
    const uint32_t up = ge_A & ~gt_Z & ~x & 0x80808080u;
    return x | (up >> 2);
}

PFAC_FOLD_FN unsigned char pfac_fold_byte(unsigned char b) {
    return (unsigned char)pfac_fold_dword(b);
}

#endif
