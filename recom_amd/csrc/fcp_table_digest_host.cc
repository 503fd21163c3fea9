// fcp_table_digest_host.cc — the host side of the table digest: fcp_table_digest_host (the digest of rows in HOST memory — a
// checkpoint before it is loaded, a table copied back) and the argument checks of the two device entries
// (fcp_table_digest.hip).  Ordinary C++, no GPU header and no other unit of the library: it links, and is tested under
// sanitizers, on its own.  The value model is fcp_table_digest.h's.
//
// Rows are read with memcpy, so host rows may start at any byte; the last word of a row is assembled from the row's own
// last 1 .. 7 bytes, so nothing outside [first_row, first_row + rows * row bytes) is read.  Words are little-endian, as
// every host this library builds for is.
#include "fcp_table_digest.h"

#include <cstring>

namespace fcpd {
namespace {

int refuse(std::string *why, const std::string &msg) {
  if (why) *why = msg;
  return FCP_ERR_INVALID_ARGUMENT;
}

// what both entries ask of kind, dim, row0 and row_step; `last` is the largest local row index + 1 (rows / table_rows)
int check_common(const std::string &w, int32_t kind, int32_t dim, int64_t row0, int64_t row_step, int64_t last, std::string *why) {
  if (dim <= 0) return refuse(why, w + "`dim` must be positive");
  if (!fcpf::known_tab_kind(kind)) return refuse(why, w + "`kind` is no FCP_TAB_* row format");
  if (fcpf::row_bytes(kind, dim) > 0x7FFFFFFF) return refuse(why, w + "`dim` gives rows of 2 GiB or more");
  if (row0 < 0) return refuse(why, w + "`row0` is negative");
  if (row_step < 1) return refuse(why, w + "`row_step` must be at least 1");
  int64_t span = 0, top = 0;
  if (last > 0 && (__builtin_mul_overflow(last - 1, row_step, &span) || __builtin_add_overflow(row0, span, &top)))
    return refuse(why, w + "`row0` + (rows - 1) * `row_step` overflows int64");
  return FCP_OK;
}

int check_aligned(const std::string &w, const char *name, const void *p, int align, const char *what, std::string *why) {
  if ((uintptr_t)p % (uintptr_t)align)
    return refuse(why, w + fcpf::not_aligned(name, align, what));
  return FCP_OK;
}

} // namespace

int check_digest(const std::string &w, const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step,
                 const void *out, const void *workspace, std::string *why) {
  if (rows < 0) return refuse(why, w + "`rows` is negative");
  if (rows >= kRowLimit) return refuse(why, w + "`rows` must stay below 2^32 - 3, a plan's row limit");
  int rc = check_common(w, kind, dim, row0, row_step, rows, why);
  if (rc) return rc;
  if (!out) return refuse(why, w + "`out` is null");
  if (!workspace) return refuse(why, w + "`workspace` is null");
  if (rows > 0 && !first_row) return refuse(why, w + "`first_row` is null");
  if ((rc = check_aligned(w, "first_row", first_row, row_alignment(kind, dim), " (a row of this kind and dim)", why))) return rc;
  if ((rc = check_aligned(w, "out", out, 8, "", why))) return rc;
  return check_aligned(w, "workspace", workspace, 8, "", why);
}

int check_digest_rows(const std::string &w, const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step,
                      const void *row_ids, int64_t n, const void *out, const void *workspace, std::string *why) {
  if (n < 0) return refuse(why, w + "`n` is negative");
  if (n >= kRowLimit) return refuse(why, w + "`n` must stay below 2^32 - 3");
  if (table_rows < 0 || table_rows >= kRowLimit) return refuse(why, w + "`table_rows` must lie in [0, 2^32 - 3), a plan's row limit");
  int rc = check_common(w, kind, dim, row0, row_step, table_rows, why);
  if (rc) return rc;
  if (!out) return refuse(why, w + "`out` is null");
  if (!workspace) return refuse(why, w + "`workspace` is null");
  if (n > 0 && table_rows > 0 && !table) return refuse(why, w + "`table` is null");
  if (n > 0 && !row_ids) return refuse(why, w + "`row_ids` is null");
  if ((rc = check_aligned(w, "table", table, row_alignment(kind, dim), " (a row of this kind and dim)", why))) return rc;
  if ((rc = check_aligned(w, "row_ids", row_ids, 8, "", why))) return rc;
  if ((rc = check_aligned(w, "out", out, 8, "", why))) return rc;
  return check_aligned(w, "workspace", workspace, 8, "", why);
}

int check_digest(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step, const void *out,
                 const void *workspace, std::string *why) {
  return check_digest("fcp_table_digest: ", first_row, kind, rows, dim, row0, row_step, out, workspace, why);
}

int check_digest_rows(const void *table, int32_t kind, int64_t table_rows, int32_t dim, int64_t row0, int64_t row_step, const void *row_ids,
                      int64_t n, const void *out, const void *workspace, std::string *why) {
  return check_digest_rows("fcp_table_digest_rows: ", table, kind, table_rows, dim, row0, row_step, row_ids, n, out, workspace, why);
}

} // namespace fcpd

extern "C" uint64_t fcp_table_digest_host(const void *first_row, int32_t kind, int64_t rows, int32_t dim, int64_t row0, int64_t row_step) {
  using namespace fcpd;
  if (rows < 0 || rows >= kRowLimit || check_common("", kind, dim, row0, row_step, rows, nullptr)) return 0;
  if (rows > 0 && !first_row) return 0;
  const int64_t rb = fcpf::row_bytes(kind, dim);
  const int64_t full = rb / 8;
  const int rem = (int)(rb % 8);
  const uint64_t salt = salt_of(kind, dim);
  const unsigned char *row = static_cast<const unsigned char *>(first_row);
  uint64_t sum = 0;
  for (int64_t i = 0; i < rows; ++i, row += rb) {
    uint64_t terms = 0, word;
    for (int64_t j = 0; j < full; ++j) {
      std::memcpy(&word, row + 8 * j, 8);
      terms += word_term(word, (uint64_t)j);
    }
    if (rem) {
      word = 0;
      std::memcpy(&word, row + 8 * full, (size_t)rem); // the row's own last bytes; the rest of the word is zero
      terms += word_term(word, (uint64_t)full);
    }
    sum += row_hash(salt, (uint64_t)row0 + (uint64_t)i * (uint64_t)row_step, terms);
  }
  return sum;
}
