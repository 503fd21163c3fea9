// table_digest_san.cc — fcp_table_digest_host and the device entries' argument checks (recom_amd/csrc/fcp_table_digest_host.cc)
// on their own, for a build with -fsanitize=address,undefined: the unit needs no GPU runtime and no other unit of the library.
//   table_digest_san CASES
// CASES: one case per line, `kind dim rows row0 step expected-hex bytes-hex` ("-" for no bytes), as
// tests/table_digest_cases.py writes them.  The rows of a case lie in a heap block of EXACTLY rows * row bytes, so a read past
// the last row is the sanitizer's to report.  Prints one line per mismatch and `<n> failures` at the end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "fcp_table_digest.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: table_digest_san CASES\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  int failures = 0, cases = 0;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream s(line);
    int kind, dim;
    long long rows, row0, step;
    std::string want_hex, bytes_hex;
    if (!(s >> kind >> dim >> rows >> row0 >> step >> want_hex >> bytes_hex)) {
      std::fprintf(stderr, "bad case line: %s\n", line.c_str());
      return 2;
    }
    const uint64_t want = std::strtoull(want_hex.c_str(), nullptr, 16);
    const size_t n = bytes_hex == "-" ? 0 : bytes_hex.size() / 2;
    if (!fcpf::known_tab_kind(kind) || dim <= 0 || (int64_t)n != rows * fcpf::row_bytes(kind, dim)) {
      std::fprintf(stderr, "case %d: %zu bytes are not %lld rows\n", cases, n, rows);
      return 2;
    }
    unsigned char *block = static_cast<unsigned char *>(std::malloc(n ? n : 1)); // (n == 0: the pointer is never read)
    for (size_t i = 0; i < n; ++i) block[i] = (unsigned char)(hexval(bytes_hex[2 * i]) << 4 | hexval(bytes_hex[2 * i + 1]));
    const uint64_t got = fcp_table_digest_host(n ? block : nullptr, kind, rows, dim, row0, step);
    if (got != want) {
      std::printf("case %d (kind %d dim %d rows %lld): got %016" PRIx64 ", want %016" PRIx64 "\n", cases, kind, dim, rows, got, want);
      ++failures;
    }
    // the same rows one byte into a larger block: host rows may start anywhere
    if (n) {
      unsigned char *odd = static_cast<unsigned char *>(std::malloc(n + 1));
      std::memcpy(odd + 1, block, n);
      if (fcp_table_digest_host(odd + 1, kind, rows, dim, row0, step) != want) {
        std::printf("case %d: another digest at an odd address\n", cases);
        ++failures;
      }
      std::free(odd);
    }
    std::free(block);
    ++cases;
  }

  // invalid arguments give 0 and read nothing
  unsigned char one[16] = {1};
  const struct { const void *p; int kind; long long rows; int dim; long long row0, step; } bad[] = {
      {nullptr, 0, 1, 1, 0, 1}, {one, 4, 1, 1, 0, 1}, {one, -1, 1, 1, 0, 1}, {one, 255, 1, 1, 0, 1}, {one, 0, 1, 0, 0, 1},
      {one, 0, -1, 1, 0, 1},    {one, 0, 1, 1, -1, 1}, {one, 0, 1, 1, 0, 0}, {one, 0, 2, 1, INT64_MAX, 1}, {one, 0, 3, 1, 0, INT64_MAX},
      {one, 0, (1ll << 32) - 3, 1, 0, 1}};
  for (const auto &b : bad)
    if (fcp_table_digest_host(b.p, b.kind, b.rows, b.dim, b.row0, b.step) != 0) {
      std::printf("invalid arguments (kind %d rows %lld dim %d row0 %lld step %lld) gave a digest\n", b.kind, b.rows, b.dim, b.row0, b.step);
      ++failures;
    }

  // the device entries' checks: a message for every refusal, none for valid arguments
  std::string why;
  const void *A = reinterpret_cast<const void *>(uintptr_t(1) << 20);
  if (fcpd::check_digest(A, 0, 5, 64, 0, 1, A, A, &why) != FCP_OK || !why.empty()) ++failures, std::printf("valid digest arguments refused\n");
  if (fcpd::check_digest(A, 0, -1, 64, 0, 1, A, A, &why) != FCP_ERR_INVALID_ARGUMENT || why.find("`rows`") == std::string::npos)
    ++failures, std::printf("negative rows: %s\n", why.c_str());
  why.clear();
  if (fcpd::check_digest_rows(A, 3, 5, 1, 0, 1, A, 4, A, A, &why) != FCP_OK || !why.empty()) ++failures, std::printf("valid by-id arguments refused\n");
  if (fcpd::check_digest_rows(A, 3, 5, 1, 0, 1, reinterpret_cast<const char *>(A) + 4, 4, A, A, &why) != FCP_ERR_INVALID_ARGUMENT ||
      why.find("`row_ids`") == std::string::npos)
    ++failures, std::printf("misaligned row_ids: %s\n", why.c_str());
  if (fcpd::check_digest(A, 0, 2, 1, INT64_MAX, 1, A, A, nullptr) != FCP_ERR_INVALID_ARGUMENT) ++failures, std::printf("overflow accepted\n");

  std::printf("%d cases\n%d failures\n", cases, failures);
  return failures ? 1 : 0;
}
