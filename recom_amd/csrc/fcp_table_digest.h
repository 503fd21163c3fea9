// fcp_table_digest.h — what the two units of the table digest share: fcp_table_digest_host.cc (ordinary C++: the host
// digest and the argument checks of the device entries) and fcp_table_digest.hip (the kernels).  The value model is stated once,
// here, in functions both compilers take; the header's text (include/fcp_hip.h) says the same in words.  No GPU header.
//
// All arithmetic is unsigned, modulo 2^64.  The digest finds ACCIDENTS — a changed byte, swapped rows or words, a row at the
// wrong index, bytes read as another kind or dim.  It is not a MAC: anyone who can choose the bytes can choose the sum.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/fcp_hip.h"
#include "fcp_formats.h"

#if defined(__HIPCC__)
#define FCP_DIGEST_FN __host__ __device__ inline
#else
#define FCP_DIGEST_FN inline
#endif

namespace fcpd {

constexpr uint64_t kGolden = 0x9e3779b97f4a7c15ull; // G
using fcpf::kRowLimit;                              // rows, n and table_rows stay below it

// the 64-bit finaliser; mix(1) == 0xb456bcfc34c2cb2c
FCP_DIGEST_FN uint64_t mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}
FCP_DIGEST_FN uint64_t salt_of(int32_t kind, int32_t dim) { return mix(((uint64_t)(uint32_t)(kind + 1) << 32) | (uint64_t)(uint32_t)dim); }
// the term of word j (from 0) of a row
FCP_DIGEST_FN uint64_t word_term(uint64_t w, uint64_t j) { return mix(w ^ ((j + 1) * kGolden)); }
// H(r): `terms` is the sum of the row's word terms, r its GLOBAL index
FCP_DIGEST_FN uint64_t row_hash(uint64_t salt, uint64_t r, uint64_t terms) { return mix(salt + (r + 1) * kGolden + terms); }

// the alignment a row of `kind` and `dim` has in a table that obeys the plans' rule: 4 * V (float32), 2 * V (bf16 / fp16), 1 (q8)
inline int row_alignment(int kind, int32_t dim) {
  if (fcpf::kTab[kind].row_tail) return 1;
  return fcpf::kTab[kind].elem * (dim % 4 == 0 ? 4 : dim % 2 == 0 ? 2 : 1);
}

// The argument checks of fcp_table_digest / fcp_table_digest_rows, in the header's order.  FCP_OK, or
// FCP_ERR_INVALID_ARGUMENT with *why naming the argument between backquotes (the caller hands it to fcp_last_error).
int check_digest(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step, const void *out,
                 const void *workspace, std::string *why);
int check_digest_rows(const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step, const void *row_ids,
                      int64_t n, const void *out, const void *workspace, std::string *why);
// The same checks behind another text: `w` goes in front of the message in place of "fcp_table_digest: " /
// "fcp_table_digest_rows: " (the grouped entry, fcp_tables_digest_plan.cc: "fcp_tables_digest: entry k: ").
int check_digest(const std::string &w, const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step,
                 const void *out, const void *workspace, std::string *why);
int check_digest_rows(const std::string &w, const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step,
                      const void *row_ids, int64_t n, const void *out, const void *workspace, std::string *why);

} // namespace fcpd
