// episode_host.hpp - what every closed-loop episode entry does with its records on the host (host code only; no HIP header is needed).
// An episode of T periods over B environments records sections [T][B][row] one behind the other in one device block, reads the block
// back once and hands the caller the rows the call wrote - and nothing else: a row the call did not write stays what the caller put there
// (NaN), n_run says how far every environment got, an environment that has stopped takes nothing further.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace dust {
// one section of the records: n rows per environment, at `off` floats from the block's start (absent: no room, off is where it would lie)
struct RecSection {
  size_t off, n, B, row;
  bool present;
  // row t of the section in the block `rec` (absent: nullptr - the kernels' "no such record")
  float *at(float *rec, size_t t) const { return present ? rec + off + t * B * row : nullptr; }
};

// The layout: sections are appended in the order the kernels find them; an absent one takes no room
struct EpisodeRecords {
  size_t T, B, n_rec = 0;
  EpisodeRecords(size_t periods, size_t n_env) : T(periods), B(n_env) {}
  // a section [n][B][row]; n: the periods, or 1 for a record of the call's end (the AMPPI episodes' final a_seq [B][D])
  RecSection add(size_t row, bool present = true, size_t n = 0) {
    RecSection s{n_rec, n ? n : T, B, row, present};
    if (present) n_rec += s.n * B * row;
    return s;
  }
  RecSection per_call(size_t row, bool present = true) { return add(row, present, 1); }
  // the rules' words [B] loss | [B] status | [B] n_run; returns where they lie
  size_t words(bool present = true) { return add(1, present, 3).off; }
  size_t total() const { return n_rec; }
};

// Row t of environment e goes from the block read back (`host`) to dst [n][B][row] if e participates (active: NULL - everybody) and
// first <= t < ran[e] (ran: NULL - every row of the section)
inline void records_scatter(float *dst, const float *host, const RecSection &s, const unsigned char *active, const int *ran, size_t first = 0) {
  const float *src = host + s.off;
  if (!active && !ran && first == 0) {
    memcpy(dst, src, s.n * s.B * s.row * sizeof(float));
    return;
  }
  for (size_t e = 0; e < s.B; ++e) {
    if (active && !active[e]) continue;
    const size_t end = !ran ? s.n : (ran[e] < 0 ? 0 : ((size_t)ran[e] < s.n ? (size_t)ran[e] : s.n));
    for (size_t t = first; t < end; ++t) memcpy(dst + (t * s.B + e) * s.row, src + (t * s.B + e) * s.row, s.row * sizeof(float));
  }
}

// One row per environment (the sequence an episode leaves behind), src [B][row] -> dst, for the participating environments that ran more
// than `beyond` periods (ran: NULL - all of them)
inline void env_rows_out(float *dst, const float *src, size_t B, size_t row, const unsigned char *active, const int *ran, size_t beyond = 0) {
  for (size_t e = 0; e < B; ++e)
    if ((!active || active[e]) && (!ran || (long long)ran[e] > (long long)beyond)) memcpy(dst + e * row, src + e * row, row * sizeof(float));
}

// What the rules' words hold when the call begins: the caller's loss and status, and n_run = 0 (an environment that enters stopped has run
// no period)
inline std::vector<float> rules_words_in(const float *loss, const int *status, size_t B) {
  std::vector<float> in(3 * B, 0.f);
  memcpy(in.data(), loss, B * sizeof(float));
  memcpy(in.data() + B, status, B * sizeof(int));
  return in;
}

// The periods every environment ran, from the words read back (`words`: where they begin); run: NULL, or who took part at all - the others
// ran none, whatever the device left in their word
inline std::vector<int> rules_ran(const float *words, size_t B, const unsigned char *run = nullptr) {
  std::vector<int> ran(B);
  memcpy(ran.data(), words + 2 * B, B * sizeof(int));
  for (size_t e = 0; e < B && run; ++e)
    if (!run[e]) ran[e] = 0;
  return ran;
}

// The words go back to the caller: n_run of every participating environment; loss and status only where a period ran (an environment that
// entered with status != 0 keeps what it came with)
inline void rules_words_out(const float *words, size_t B, const unsigned char *active, const int *ran, float *loss, int *status, int *n_run) {
  for (size_t e = 0; e < B; ++e) {
    if (active && !active[e]) continue;
    n_run[e] = ran[e];
    if (ran[e] == 0) continue;
    memcpy(loss + e, words + e, sizeof(float));
    memcpy(status + e, words + B + e, sizeof(int));
  }
}
}  // namespace dust
