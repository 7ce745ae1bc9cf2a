// rec_tables_check.cpp -- the .rec coder's core over empirical symbol tables (csrc/irec_rec_core.h: TableModel, Tables) under the host
// sanitizers.  A stand-alone program in the pattern of scripts/rec_core_check.cpp: every line of the core that the kernels of
// csrc/irec_rec.hip run is compiled here by g++ and runs with AddressSanitizer and UndefinedBehaviorSanitizer.  Build and run
// from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Irelative-entropy-coding_amd/csrc \
//       scripts/rec_tables_check.cpp -o /tmp/rec_tables_check -lpthread && /tmp/rec_tables_check
// It walks the layouts and tables of tests/rec_tables_cases.py (index only, counts only, both; contiguous and strided input; a short cap)
// with every buffer -- the tables too -- sized EXACTLY, so that one byte, one index or one table entry past a range is a report; reads
// every call's files back and compares the rows; checks each stream against irec_ac_encode over the same counts (irec_io.cpp, the coder
// that tests/golden/rec_ac_vectors.npz pins to the compiled reference); hands hostile tables to both directions; and reads a damaged
// set of flagged files.  Exit status 0 and the last line "rec_tables_check: all equal" mean: round trips exact, streams equal to
// irec_io.cpp's, IREC_REC_E_TABLE for every hostile table, and no sanitizer report (profiles/rec_tables/sanitizer_core.log is this
// program's output).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "irec_io.cpp"
#include "irec_rec_core.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { g_state += 0x9E3779B97F4A7C15ull; uint64_t z = g_state; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }
int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

constexpr int32_t MAX_K = 9;

struct TableSet {   // exactly-sized arrays; empty vectors = no table of that kind
  std::vector<int64_t> index_counts; std::vector<std::vector<int64_t>> count_counts;
  std::vector<uint32_t> index_cum, count_cum; std::vector<int32_t> count_first;
  irec_rec::Tables view() const {
    return irec_rec::Tables{index_cum.empty() ? nullptr : index_cum.data(), index_cum.empty() ? 0 : (int32_t)index_cum.size() - 1,
                            count_cum.empty() ? nullptr : count_cum.data(), count_first.empty() ? nullptr : count_first.data(), (int64_t)count_cum.size()};
  }
};
std::vector<uint32_t> cumulate(const std::vector<int64_t> &c) {
  std::vector<uint32_t> cum(c.size() + 1, 0);
  for (size_t m = 0; m < c.size(); ++m) cum[m + 1] = cum[m] + (uint32_t)c[m];
  return cum;
}
TableSet make_tables(const std::vector<int64_t> &index_counts, int32_t R, bool counts) {
  TableSet t;
  t.index_counts = index_counts;
  if (!index_counts.empty()) t.index_cum = cumulate(index_counts);
  if (counts) {
    const int lengths[3] = {11, 3, 16};
    t.count_first.push_back(0);
    for (int32_t r = 0; r < R; ++r) {
      std::vector<int64_t> c{3};
      for (int m = 0; m < lengths[r % 3] - 1; ++m) c.push_back((256 >> m) > 1 ? (256 >> m) : 1);
      const std::vector<uint32_t> cum = cumulate(c);
      t.count_counts.push_back(c);
      t.count_cum.insert(t.count_cum.end(), cum.begin(), cum.end());
      t.count_first.push_back((int32_t)t.count_cum.size());
    }
  }
  return t;
}

struct Rows { int32_t N; std::vector<int32_t> bpr, K, idx; int64_t T; };
Rows make_rows(int32_t N, const std::vector<int32_t> &bpr, const TableSet &t, bool zero) {
  Rows p{N, bpr, {}, {}, 0};
  for (int32_t b : bpr) p.T += b;
  p.K.resize((size_t)(N * p.T)); p.idx.resize((size_t)(N * p.T * MAX_K));
  const int lengths[3] = {11, 3, 16};
  const int64_t n_values = t.index_counts.empty() ? 20 : (int64_t)t.index_counts.size() - 1;
  for (int32_t i = 0; i < N; ++i) {
    int64_t b = 0;
    for (size_t r = 0; r < bpr.size(); ++r)
      for (int32_t j = 0; j < bpr[r]; ++j, ++b) {
        int32_t k = below(7) == 0 ? 0 : (int32_t)below(MAX_K + 1);
        if (!t.count_counts.empty() && k > lengths[r % 3] - 2) k = lengths[r % 3] - 2;
        p.K[(size_t)(i * p.T + b)] = zero ? 0 : k;
      }
  }
  for (auto &v : p.idx) v = (int32_t)below(n_values);
  if (!zero) { p.K[0] = MAX_K; p.idx[0] = (int32_t)n_values - 1; }
  return p;
}

void core_encode(const Rows &p, uint32_t S, const irec_rec::Tables &tb, bool strided, int64_t cap, std::vector<uint8_t> &out, std::vector<int64_t> &off,
                 std::vector<int32_t> &status) {
  std::vector<int32_t> joined;
  const int32_t *K = p.K.data(), *idx = p.idx.data();
  int64_t ks = 1, is = MAX_K;
  if (strided) {
    const size_t rows = p.K.size();
    joined.resize(rows * (1 + (size_t)MAX_K));
    for (size_t b = 0; b < rows; ++b) { joined[b * (1 + MAX_K)] = p.K[b]; for (int32_t t = 0; t < MAX_K; ++t) joined[b * (1 + MAX_K) + 1 + t] = p.idx[b * MAX_K + t]; }
    K = joined.data(); idx = joined.data() + 1; ks = is = 1 + MAX_K;
  }
  const int32_t R = (int32_t)p.bpr.size();
  out.assign((size_t)cap, 0xAB); off.assign((size_t)p.N + 1, -1); status.assign((size_t)p.N, -1);
  std::vector<uint8_t> ws((size_t)irec_rec::encode_workspace_bytes(p.N, R));
  irec_rec::EncodeCall c{42, 1000, S, 32, 48, 3, p.N, R, 0, MAX_K, K, ks, idx, is, out.data(), cap, off.data(), status.data(), nullptr, nullptr, nullptr, {}};
  CHECK(irec_rec::ragged_first(R, p.bpr.data(), c.first));
  irec_rec::encode_bind_workspace(c, ws.data());
  irec_rec::encode_call_host(c, tb);
}

void core_decode(const std::vector<uint8_t> &blob, const std::vector<int64_t> &off, const std::vector<int32_t> &bpr, int32_t mk, const irec_rec::Tables &tb,
                 std::vector<uint32_t> &hdr, std::vector<int32_t> &K, std::vector<int32_t> &idx, std::vector<int32_t> &status) {
  const int32_t N = (int32_t)off.size() - 1, R = (int32_t)bpr.size();
  int64_t T = 0;
  for (int32_t b : bpr) T += b;
  hdr.assign((size_t)N * 9, 0xFFFFFFFFu); K.assign((size_t)(N * T), -1); idx.assign((size_t)(N * T * mk), -1); status.assign((size_t)N, -1);
  std::vector<int32_t> ws((size_t)(irec_rec::decode_workspace_bytes(N, R) / 4));
  std::vector<uint8_t> exact(blob.begin(), blob.end());                  // (exactly the blob's size: a read past the last file is a report)
  irec_rec::DecodeCall c{exact.data(), off.data(), N, R, 0, mk, hdr.data(), K.data(), idx.data(), status.data(), ws.data(), {}};
  CHECK(irec_rec::ragged_first(R, bpr.data(), c.first));
  irec_rec::decode_call_host(c, tb);
}

// the count stream of (image 0, residual block 0) and its index stream, cut from the file, against irec_ac_encode + irec_rec_pack_bits
void check_streams_against_io(const Rows &p, const TableSet &t, uint32_t S, const std::vector<uint8_t> &blob) {
  const int32_t R = (int32_t)p.bpr.size();
  const uint8_t *f = blob.data(), *dyn = f + 28;
  auto coded = [&](const std::vector<int64_t> &counts, const std::vector<int64_t> &values) {
    std::vector<int64_t> msg;
    for (int64_t v : values) msg.push_back(v + 1);
    msg.push_back(0);
    std::vector<uint8_t> bits(64 + 64 * msg.size()), bytes;
    int64_t n_bits = 0;
    CHECK(irec_ac_encode(counts.data(), (int32_t)counts.size(), msg.data(), (int64_t)msg.size(), 32, bits.data(), (int64_t)bits.size(), &n_bits) == IREC_OK);
    bytes.resize((size_t)((n_bits + 8) / 8));
    CHECK(irec_rec_pack_bits(bits.data(), n_bits, bytes.data(), (int64_t)bytes.size()) == (int64_t)bytes.size());
    return bytes;
  };
  auto uniform = [](int64_t n_values, int64_t w) { std::vector<int64_t> c((size_t)n_values + 1, 1 + w); c[0] = 1; return c; };
  int64_t c_at = 28 + 16 * R, x_at = c_at;
  for (int32_t q = 0; q < R; ++q) x_at += irec_rec::get_u32(dyn + 4 * (R + q));
  std::vector<int64_t> ks, xs;
  int32_t mx = 0;
  for (int32_t j = 0; j < p.bpr[0]; ++j) {
    ks.push_back(p.K[(size_t)j]); mx = p.K[(size_t)j] > mx ? p.K[(size_t)j] : mx;
    for (int32_t q = 0; q < p.K[(size_t)j]; ++q) xs.push_back(p.idx[(size_t)j * MAX_K + q]);
  }
  const std::vector<uint8_t> cs = coded(t.count_counts.empty() ? uniform(mx + 1, 100) : t.count_counts[0], ks);
  const std::vector<uint8_t> is = coded(t.index_counts.empty() ? uniform(S, 1000) : t.index_counts, xs);
  CHECK(irec_rec::get_u32(dyn + 4 * R) == cs.size() && std::equal(cs.begin(), cs.end(), f + c_at));
  CHECK(irec_rec::get_u32(dyn + 8 * R) == is.size() && std::equal(is.begin(), is.end(), f + x_at));
  CHECK(irec_rec::get_u16(f + 22) == (t.count_counts.empty() ? 0u : 1u) && irec_rec::get_u16(f + 24) == (t.index_counts.empty() ? 0u : 1u));
  CHECK(irec_rec::get_u32(dyn + 12 * R) == (t.count_counts.empty() ? (uint32_t)mx : 0xFFFFFFFFu));
}

void check_case(const char *name, int32_t N, const std::vector<int32_t> &bpr, const std::vector<int64_t> &index_counts, bool counts, bool zero = false) {
  const TableSet t = make_tables(index_counts, (int32_t)bpr.size(), counts);
  const Rows p = make_rows(N, bpr, t, zero);
  const uint32_t S = index_counts.empty() ? 20u : (uint32_t)index_counts.size() - 1;
  std::vector<uint8_t> out, ref; std::vector<int64_t> off, ref_off; std::vector<int32_t> status;
  core_encode(p, S, t.view(), false, 1 << 22, ref, ref_off, status);
  for (int32_t s : status) CHECK(s == 0);
  const int64_t total = ref_off[(size_t)N];
  ref.resize((size_t)total);
  for (int strided = 0; strided < 2; ++strided) {
    core_encode(p, S, t.view(), strided != 0, total, out, off, status);    // exactly enough room
    CHECK(out == ref); CHECK(off == ref_off);
  }
  core_encode(p, S, t.view(), false, total - 1, out, off, status);        // one byte short: nothing written, the size reported
  CHECK(off[(size_t)N] == total);
  for (uint8_t b : out) if (b != 0xAB) { CHECK(b == 0xAB); break; }
  check_streams_against_io(p, t, S, ref);
  std::vector<uint32_t> hdr; std::vector<int32_t> K, idx;
  core_decode(ref, ref_off, bpr, MAX_K, t.view(), hdr, K, idx, status);
  for (int32_t s : status) CHECK(s == 0);
  CHECK(K == p.K);
  for (size_t b = 0; b < p.K.size(); ++b)
    for (int32_t q = 0; q < MAX_K; ++q) CHECK(idx[b * MAX_K + q] == (q < p.K[b] ? p.idx[b * MAX_K + q] : 0));
  core_decode(ref, ref_off, bpr, MAX_K, irec_rec::Tables{nullptr, 0, nullptr, nullptr, 0}, hdr, K, idx, status);   // flagged, and no table
  for (int32_t s : status) CHECK(s == IREC_REC_E_COUNT_FILES);
  std::printf("%-28s %d images, %lld bytes: encode (contiguous, strided, short cap), streams equal to irec_io.cpp, decode exact\n", name, N, (long long)total);
}

void check_hostile() {
  const uint32_t tables[6][4] = {{1, 5, 9, 12}, {0, 5, 5, 12}, {0, 9, 5, 12}, {0, 5, 9, (1u << 30) + 1}, {0, 0, 0, 0}, {0, 5, 9, 3}};
  const bool certain_on_read[6] = {true, false, false, true, true, true};
  const std::vector<int32_t> bpr{3, 3};
  const TableSet good = make_tables({4, 5, 3}, 2, false);
  Rows p = make_rows(3, bpr, good, false);
  for (size_t b = 0; b < p.K.size(); ++b) p.K[b] = (int32_t)(b % 2 == 0);
  for (size_t e = 0; e < p.idx.size(); ++e) p.idx[e] = (int32_t)(e / MAX_K % 4 == 0 ? 1 : 0);
  TableSet good_counts = good;
  good_counts.count_cum = {0, 4, 9, 12, 0, 4, 9, 12}; good_counts.count_first = {0, 4, 8};
  std::vector<uint8_t> files, out; std::vector<int64_t> files_off, off; std::vector<int32_t> status;
  core_encode(p, 2, good_counts.view(), false, 4096, files, files_off, status);
  for (int32_t s : status) CHECK(s == 0);
  files.resize((size_t)files_off[3]);
  for (int h = 0; h < 6; ++h) {
    const std::vector<uint32_t> one(tables[h], tables[h] + 4);           // exactly 4 entries: 3 symbols
    std::vector<uint32_t> two(one); two.insert(two.end(), one.begin(), one.end());
    const std::vector<int32_t> first{0, 4, 8};
    const irec_rec::Tables as_index{one.data(), 3, nullptr, nullptr, 0}, as_counts{nullptr, 0, two.data(), first.data(), 8};
    for (const irec_rec::Tables &tb : {as_index, as_counts}) {
      core_encode(p, 2, tb, false, 4096, out, off, status);
      for (int32_t s : status) CHECK(s == IREC_REC_E_TABLE);
      CHECK(off[3] == 0);
    }
    std::vector<uint32_t> hdr; std::vector<int32_t> K, idx;
    const irec_rec::Tables r1{one.data(), 3, good_counts.count_cum.data(), good_counts.count_first.data(), 8},
        r2{good.index_cum.data(), 3, two.data(), first.data(), 8};
    for (const irec_rec::Tables &tb : {r1, r2}) {
      core_decode(files, files_off, bpr, MAX_K, tb, hdr, K, idx, status);
      for (int32_t s : status) { CHECK(s >= 0 && s <= IREC_REC_E_TABLE); if (certain_on_read[h]) CHECK(s == IREC_REC_E_TABLE); }
    }
  }
  const int32_t firsts[4][3] = {{0, 4, 9}, {0, 0, 4}, {-1, 4, 8}, {4, 0, 8}};
  for (int h = 0; h < 4; ++h) {
    const std::vector<int32_t> first(firsts[h], firsts[h] + 3);
    const irec_rec::Tables tb{good.index_cum.data(), 3, good_counts.count_cum.data(), first.data(), 8};
    core_encode(p, 2, tb, false, 4096, out, off, status);
    for (int32_t s : status) CHECK(s == IREC_REC_E_TABLE);
    std::vector<uint32_t> hdr; std::vector<int32_t> K, idx;
    core_decode(files, files_off, bpr, MAX_K, tb, hdr, K, idx, status);
    for (int32_t s : status) CHECK(s == IREC_REC_E_TABLE);
  }
  std::printf("hostile tables: 6 cumulative arrays as index and as count tables, 4 count_first arrays: IREC_REC_E_TABLE, and every call returned\n");
}

void check_damaged() {
  const std::vector<int32_t> bpr(6, 9);
  std::vector<int64_t> index_counts;
  for (int m = 0; m < 37; ++m) index_counts.push_back(1 + below(199));
  TableSet t = make_tables(index_counts, 6, true);
  Rows p = make_rows(1, bpr, t, false);
  std::vector<uint8_t> data; std::vector<int64_t> o2; std::vector<int32_t> status;
  core_encode(p, 36, t.view(), false, 1 << 16, data, o2, status);
  CHECK(status[0] == 0);
  const int64_t n = o2[1];
  data.resize((size_t)n);
  std::vector<std::vector<uint8_t>> files;
  for (int64_t k = 0; k < n; ++k) files.emplace_back(data.begin(), data.begin() + k);
  for (int c = 0; c < 800; ++c) {
    std::vector<uint8_t> b = data;
    for (int64_t q = 1 + below(3); q > 0; --q) b[(size_t)below(n)] = (uint8_t)below(256);
    files.push_back(b);
  }
  const int fields[18] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21};
  for (int c = 0; c < 200; ++c) { std::vector<uint8_t> b = data; b[(size_t)fields[below(18)]] = (uint8_t)below(256); files.push_back(b); }
  std::vector<uint8_t> blob; std::vector<int64_t> off{0};
  for (auto &f : files) { blob.insert(blob.end(), f.begin(), f.end()); off.push_back((int64_t)blob.size()); }
  std::vector<uint32_t> hdr; std::vector<int32_t> K, idx;
  core_decode(blob, off, bpr, MAX_K, t.view(), hdr, K, idx, status);
  int64_t accepted = 0, rejected = 0;
  const size_t nK = 54, nI = nK * MAX_K;
  for (size_t f = 0; f < files.size(); ++f) {
    CHECK(status[f] >= 0 && status[f] <= IREC_REC_E_TABLE);
    if (status[f] == 0) { ++accepted; continue; }
    ++rejected;
    for (size_t e = 0; e < 9; ++e) CHECK(hdr[9 * f + e] == 0);
    for (size_t e = 0; e < nK; ++e) CHECK(K[nK * f + e] == 0);
    for (size_t e = 0; e < nI; ++e) CHECK(idx[nI * f + e] == 0);
  }
  CHECK(accepted >= 100 && rejected >= n + 300);
  std::printf("damaged set: %zu files of a %lld-byte flagged container, %lld accepted, %lld rejected with zeroed outputs\n", files.size(), (long long)n,
              (long long)accepted, (long long)rejected);
}
} // namespace

int main() {
  std::vector<int64_t> geo{7}, ones(21, 1), lds, lds1;
  for (int m = 1; m <= 20; ++m) geo.push_back(((1 << 20) >> m) > 1 ? ((1 << 20) >> m) : 1);
  for (int m = 0; m < IREC_REC_TABLE_LDS_SYMBOLS + 1; ++m) { lds1.push_back(1 + below(64)); if (m < IREC_REC_TABLE_LDS_SYMBOLS) lds.push_back(lds1.back()); }
  const std::vector<int32_t> l1{1}, l33{3, 3}, l417{4, 1, 7}, l222{2, 2, 2}, l64(64, 1);
  const struct { const char *name; int32_t N; const std::vector<int32_t> *bpr; bool zero; } layouts[6] = {
      {"1x1", 1, &l1, false}, {"3x3_3", 3, &l33, false}, {"5x4_1_7", 5, &l417, false}, {"70x2_2_2", 70, &l222, false}, {"2x64ones", 2, &l64, false},
      {"zeroK", 3, &l33, true}};
  for (const auto &l : layouts) {
    char name[64];
    std::snprintf(name, sizeof name, "%s-index", l.name);  check_case(name, l.N, *l.bpr, geo, false, l.zero);
    std::snprintf(name, sizeof name, "%s-counts", l.name); check_case(name, l.N, *l.bpr, {}, true, l.zero);
    std::snprintf(name, sizeof name, "%s-both", l.name);   check_case(name, l.N, *l.bpr, geo, true, l.zero);
  }
  check_case("3x3_3-index-one", 3, l33, {1, 5}, false);
  check_case("3x3_3-index-ones20", 3, l33, ones, false);
  check_case("3x3_3-index-total2p30", 3, l33, {1, (1 << 30) - 3, 1, 1}, false);
  check_case("3x3_3-index-lds", 3, l33, lds, false);
  check_case("3x3_3-index-lds_plus1", 3, l33, lds1, false);
  check_hostile();
  check_damaged();
  if (g_failures) { std::printf("rec_tables_check: %d FAILED\n", g_failures); return 1; }
  std::printf("rec_tables_check: all equal\n");
  return 0;
}
