// episode_host_check.cpp - csrc/episode_host.hpp on the CPU: the record layouts of the five episode entries against the closed forms their
// pointer arithmetic had, the scatter of the rows a call wrote against a naive triple loop, the rules' words.  Built with
// -fsanitize=address,undefined and run as a child process (tests/test_episode_host_cpu.py).  Exit status 0 and "episode_host ok" on
// success; the first failed check prints its line and exits 1 (a read or write out of bounds is the sanitizer's to report).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "episode_host.hpp"
using namespace dust;

#define CHECK(x)                             \
  do {                                       \
    if (!(x)) {                              \
      printf("line %d: %s\n", __LINE__, #x); \
      exit(1);                               \
    }                                        \
  } while (0)

static const size_t T = 3, B = 4, ds = 2, da = 1, N = 3, S = 5, D = 4;

// ---- the layouts: every entry's section list, with and without every optional section
static void amppi_layouts() {  // dust_amppi_batch_episode; with bw: dust_amppi_dual_batch_episode (rec_q follows the bandwidths)
  for (int m = 0; m < 16; ++m) {
    const bool co = m & 1, om = m & 2, bw = m & 4, q = m & 8;
    EpisodeRecords lay(T, B);
    const RecSection s = lay.add(ds), a = lay.add(da), c = lay.add(S, co), o = lay.add(S, om), w = lay.add(1, bw), qq = lay.per_call(D, q);
    const size_t rec_a = T * B * ds, rec_c = rec_a + T * B * da, rec_o = rec_c + (co ? T * B * S : 0), rec_bw = rec_o + (om ? T * B * S : 0),
                 rec_q = rec_bw + (bw ? T * B : 0);
    CHECK(s.off == 0 && a.off == rec_a && c.off == rec_c && o.off == rec_o && w.off == rec_bw && qq.off == rec_q);
    CHECK(lay.total() == T * B * (ds + da + (co ? S : 0) + (om ? S : 0) + (bw ? 1 : 0)) + (q ? B * D : 0));
    CHECK(s.n == T && qq.n == 1 && qq.row == D && qq.B == B);
    CHECK(c.present == co && o.present == om && w.present == bw && qq.present == q);
    std::vector<float> block_v(lay.total() + 1);
    float *base = block_v.data();
    CHECK(a.at(base, 2) == base + rec_a + 2 * B * da);
    CHECK((c.at(base, 1) == nullptr) == !co && (qq.at(base, 0) == nullptr) == !q);
    if (co) CHECK(c.at(base, 1) == base + rec_c + B * S);
  }
}
static void svmpc_layouts() {  // svb_episode_call; with bw: svb_dual_episode_call; without pw and bw: dust_disco_batch_episode
  for (int m = 0; m < 8; ++m) {
    const bool pw = m & 1, bw = m & 2, rules = m & 4;
    EpisodeRecords lay(T, B);
    const RecSection s = lay.add(ds), a = lay.add(da), p = lay.add(N, pw), w = lay.add(1, bw), c = lay.add(1, rules);
    const size_t words = lay.words(rules);
    const size_t rec_a = T * B * ds, rec_pw = rec_a + T * B * da, rec_bw = rec_pw + (pw ? T * B * N : 0), rec_c = rec_bw + (bw ? T * B : 0);
    CHECK(s.off == 0 && a.off == rec_a && p.off == rec_pw && w.off == rec_bw && c.off == rec_c);
    CHECK(words == T * B * (ds + da + (pw ? N : 0) + (bw ? 1 : 0) + (rules ? 1 : 0)));
    CHECK(lay.total() == words + (rules ? 3 * B : 0));
    if (!bw) {  // the plain SVMPC entry's own forms
      const size_t n_pw = pw ? T * B * N : 0, n_cost = rules ? T * B : 0;
      CHECK(c.off == T * B * (ds + da) + n_pw && words == T * B * (ds + da) + n_pw + n_cost);
    }
    if (!bw && !pw) {  // MultiDISCO's
      const size_t n_cost = rules ? T * B : 0;
      CHECK(c.off == T * B * (ds + da) && words == T * B * (ds + da) + n_cost && lay.total() == words + (rules ? 3 * B : 0));
    }
  }
}

// ---- the scatter
static const float SENTINEL = -77.f;
static std::vector<float> block(size_t n) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (float)(i + 1);
  return v;
}
static void scatter_case(size_t t_n, size_t b_n, size_t lead, size_t row, const unsigned char *active, const int *ran, size_t first) {
  EpisodeRecords lay(t_n, b_n);
  lay.add(lead);  // a section ahead, so that the offset counts
  const RecSection s = lay.add(row);
  const std::vector<float> host = block(lay.total());
  std::vector<float> got(t_n * b_n * row, SENTINEL), want(got);
  records_scatter(got.data(), host.data(), s, active, ran, first);
  size_t written = 0;
  for (size_t t = 0; t < t_n; ++t)
    for (size_t e = 0; e < b_n; ++e)
      for (size_t k = 0; k < row; ++k) {
        const bool permitted = (!active || active[e]) && t >= first && t < (ran ? (size_t)ran[e] : t_n);
        if (permitted) want[(t * b_n + e) * row + k] = host[t_n * b_n * lead + (t * b_n + e) * row + k], ++written;
      }
  CHECK(got == want);
  size_t kept = 0;
  for (float v : got) kept += v == SENTINEL;
  CHECK(kept + written == got.size());
}
static void scatters() {
  const unsigned char one_off[4] = {1, 0, 1, 1}, all_on[4] = {1, 1, 1, 1};
  const int ran[4] = {0, 1, (int)T, 2};
  for (size_t row : {(size_t)1, ds, N}) {
    scatter_case(T, B, ds, row, one_off, nullptr, 0);  // one inactive environment
    scatter_case(T, B, ds, row, nullptr, ran, 0);      // stopped environments
    scatter_case(T, B, ds, row, all_on, ran, 0);
    scatter_case(T, B, ds, row, one_off, ran, 0);
    scatter_case(T, B, ds, row, nullptr, ran, 2);  // a section whose rows begin behind the warm-up
    scatter_case(T, B, ds, row, one_off, ran, 2);
    scatter_case(T, B, ds, row, nullptr, nullptr, 2);
    scatter_case(T, B, ds, row, nullptr, nullptr, 0);  // the single copy
  }
  const unsigned char on1[1] = {1}, off1[1] = {0};
  const int ran1[1] = {1}, ran0[1] = {0};
  scatter_case(1, 1, 1, 1, nullptr, nullptr, 0);  // the edges: T = 1, B = 1, row width 1
  scatter_case(1, 1, 1, 1, on1, ran1, 0);
  scatter_case(1, 1, 1, 1, on1, ran0, 0);
  scatter_case(1, 1, 1, 1, off1, ran1, 0);
  scatter_case(1, B, 1, 1, one_off, nullptr, 0);
  scatter_case(T, 1, 1, 1, nullptr, ran1, 0);
  scatter_case(T, 1, 1, D, on1, nullptr, 1);
  // a record of the call's end, [1][B][D]
  EpisodeRecords lay(T, B);
  lay.add(ds);
  const RecSection q = lay.per_call(D);
  const std::vector<float> host = block(lay.total());
  std::vector<float> got(B * D, SENTINEL);
  records_scatter(got.data(), host.data(), q, one_off, nullptr);
  for (size_t e = 0; e < B; ++e)
    for (size_t k = 0; k < D; ++k) CHECK(got[e * D + k] == (one_off[e] ? host[T * B * ds + e * D + k] : SENTINEL));
}
static void env_rows() {
  const unsigned char one_off[4] = {1, 0, 1, 1};
  const int ran[4] = {0, 1, (int)T, 2};
  const std::vector<float> src = block(B * D);
  for (size_t beyond : {(size_t)0, (size_t)1, (size_t)2})
    for (int m = 0; m < 4; ++m) {
      const unsigned char *active = (m & 1) ? one_off : nullptr;
      const int *r = (m & 2) ? ran : nullptr;
      std::vector<float> got(B * D, SENTINEL);
      env_rows_out(got.data(), src.data(), B, D, active, r, beyond);
      for (size_t e = 0; e < B; ++e) {
        const bool permitted = (!active || active[e]) && (!r || (size_t)r[e] > beyond);
        for (size_t k = 0; k < D; ++k) CHECK(got[e * D + k] == (permitted ? src[e * D + k] : SENTINEL));
      }
    }
}

// ---- the rules' words
static void words_case(size_t b_n, const unsigned char *active, const unsigned char *run, const int *dev_ran) {
  std::vector<float> loss_in(b_n);
  std::vector<int> status_in(b_n);
  for (size_t e = 0; e < b_n; ++e) loss_in[e] = 0.5f + (float)e, status_in[e] = (int)(e % 3);
  std::vector<float> img = rules_words_in(loss_in.data(), status_in.data(), b_n);
  CHECK(img.size() == 3 * b_n);
  CHECK(!memcmp(img.data(), loss_in.data(), b_n * sizeof(float)) && !memcmp(img.data() + b_n, status_in.data(), b_n * sizeof(int)));
  const std::vector<int> zero(b_n, 0);  // n_run = 0: the kernels read the word as an int
  CHECK(!memcmp(img.data() + 2 * b_n, zero.data(), b_n * sizeof(int)));
  // what a device would leave: new losses and statuses, and the periods run
  std::vector<float> loss_dev(b_n);
  std::vector<int> status_dev(b_n);
  for (size_t e = 0; e < b_n; ++e) loss_dev[e] = 100.f + (float)e, status_dev[e] = (int)((e + 1) % 3);
  memcpy(img.data(), loss_dev.data(), b_n * sizeof(float));
  memcpy(img.data() + b_n, status_dev.data(), b_n * sizeof(int));
  memcpy(img.data() + 2 * b_n, dev_ran, b_n * sizeof(int));
  const std::vector<int> ran = rules_ran(img.data(), b_n, run);
  for (size_t e = 0; e < b_n; ++e) CHECK(ran[e] == (run && !run[e] ? 0 : dev_ran[e]));
  std::vector<float> loss(b_n, SENTINEL);
  std::vector<int> status(b_n, -5), n_run(b_n, -1);
  rules_words_out(img.data(), b_n, active, ran.data(), loss.data(), status.data(), n_run.data());
  for (size_t e = 0; e < b_n; ++e) {
    const bool part = !active || active[e];
    CHECK(n_run[e] == (part ? ran[e] : -1));
    CHECK(loss[e] == (part && ran[e] > 0 ? loss_dev[e] : SENTINEL));
    CHECK(status[e] == (part && ran[e] > 0 ? status_dev[e] : -5));
  }
}
static void words() {
  const unsigned char one_off[4] = {1, 0, 1, 1}, run[4] = {1, 1, 0, 1};
  const int ran[4] = {0, 1, (int)T, 2};
  words_case(B, nullptr, nullptr, ran);
  words_case(B, one_off, nullptr, ran);
  words_case(B, one_off, run, ran);  // the dual simulation: the words go to `active`, the periods count for the run mask
  words_case(B, nullptr, run, ran);
  const unsigned char on1[1] = {1};
  const int r1[1] = {1}, r0[1] = {0};
  words_case(1, nullptr, nullptr, r1);
  words_case(1, on1, nullptr, r0);
}

int main() {
  amppi_layouts();
  svmpc_layouts();
  scatters();
  env_rows();
  words();
  printf("episode_host ok\n");
  return 0;
}
