"""prisim_amd/csrc_addon/addon_plan.h, the planning arithmetic of the add-on entries, compiled on its own by the host compiler and
checked against the loops and formulas that the entries used to write out by hand."""
import os
import subprocess

import numpy as NP

from prisim_amd import dsp_readings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include "addon_plan.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>

using namespace pint;

int main() {
  long bad = 0, checked = 0;
  // the power-of-two test as runs.hip, subband.hip, cpdelay.hip and cpft.hip wrote it
  for (int64_t m = 1; m <= 4097; ++m) {
    int logm = 0;
    while ((int64_t(1) << logm) < m) ++logm;
    const bool pow2 = (int64_t(1) << logm) == m;
    bool got_pow2 = !pow2;
    const int got = ceil_log2(m, got_pow2);
    if (got != logm || got_pow2 != pow2) {
      std::printf("ceil_log2(%lld): %d %d, the loop %d %d\n", (long long)m, got, (int)got_pow2, logm, (int)pow2);
      ++bad;
    }
    ++checked;
  }
  // the chunk plan as the entries wrote it, with cpft.hip's guard of the byte count
  const int64_t ns[] = {1, 2, 3, 5, 64, int64_t(1) << 30};
  const int64_t pers[] = {0, 1, 24, int64_t(1) << 20, int64_t(1) << 33};
  const int64_t budgets[] = {0, 1, 47, 48, 49, int64_t(1) << 30, int64_t(1) << 40};
  const int streams[] = {1, 2};
  for (int64_t n : ns)
    for (int64_t per_item : pers)
      for (int64_t budget_bytes : budgets)
        for (int kMaxStreams : streams) {
          const int64_t budget = budget_bytes > 0 ? budget_bytes : int64_t(1) << 30;
          const int64_t tc = std::max<int64_t>(1, std::min<int64_t>(n, budget / (kMaxStreams * std::max<int64_t>(per_item, 1))));
          const int64_t nchunks = (n + tc - 1) / tc, last = n - (nchunks - 1) * tc;
          const int nstreams = (int)std::min<int64_t>(kMaxStreams, nchunks);
          const Chunks c = plan_chunks(n, per_item, budget_bytes, kMaxStreams);
          const bool same = c.size == tc && c.count == nchunks && c.last == last && c.nstreams == nstreams;
          const bool sound = c.size * (c.count - 1) + c.last == n && 1 <= c.last && c.last <= c.size && c.nstreams <= c.count &&
                             1 <= c.nstreams;
          // the same chunks again from their size, as the entries with a grid limit ask for them
          const Chunks d = chunks_of(n, c.size, kMaxStreams);
          const bool again = d.size == c.size && d.count == c.count && d.last == c.last && d.nstreams == c.nstreams;
          if (!same || !sound || !again) {
            std::printf("plan_chunks(%lld, %lld, %lld, %d): {%lld, %lld, %lld, %d}, by hand {%lld, %lld, %lld, %d}\n", (long long)n,
                        (long long)per_item, (long long)budget_bytes, kMaxStreams, (long long)c.size, (long long)c.count,
                        (long long)c.last, c.nstreams, (long long)tc, (long long)nchunks, (long long)last, nstreams);
            ++bad;
          }
          ++checked;
        }
  // a size below the plan's, as a grid limit gives it: five items in chunks of two
  const Chunks e = chunks_of(5, 2, 2);
  if (e.size != 2 || e.count != 3 || e.last != 1 || e.nstreams != 2) ++bad;
  ++checked;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def test_addon_plan_matches_the_handwritten_arithmetic(tmp_path):
    src = tmp_path / 'plan_check.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'plan_check'
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src),
                           '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert out.strip().splitlines()[-1] == 'checked %d bad 0' % (4097 + 6 * 5 * 7 * 2 + 1), out


# ---- the resampling plan and the snapshot tile ---------------------------------------------------------------------------------

CASES = [(16, 5, 16), (16, 8, 12), (12, 5, 12), (12, 16, 9), (1, 1, 1), (8, 1, 8), (4096, 256, 2048)]   # (m, nout, nchan)
NUMERIC = [(16, 5, 12), (12, 16, 9)]
DF = 1e5

RESAMPLE_PROGRAM = r'''
#include "addon_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace pint;

struct Map {
  int64_t m, nout, nchan;
  std::vector<int64_t> mo, mi;
  std::vector<double> mw;
};

// ---- by hand: the loops as the entries wrote them before addon_plan.h had them ----

// addon_internal.h: build_resample_tables
const char* hand_tables(int64_t nout, int64_t m, int64_t nchan, double scale, int64_t nmap, const int64_t* map_out, const int64_t* map_in,
                        const double* map_w, std::vector<int32_t>& rs_in, std::vector<double>& rs_c, std::vector<double>& rtw) {
  const int64_t nr = std::max<int64_t>(nout, 1);
  rs_in.assign(2 * (size_t)nr, -1);
  rs_c.assign(4 * (size_t)nr, 0.0);
  rtw.assign(2 * (size_t)nr, 0.0);
  if (nout < 1) return nullptr;
  if (nmap < 1 || !map_out || !map_in || !map_w) return "the resampled spectra need the selection map";
  std::vector<int> used((size_t)nout, 0);
  const int64_t half = m / 2;
  for (int64_t e = 0; e < nmap; ++e) {
    const int64_t k = map_out[e], kin = map_in[e];
    if (k < 0 || k >= nout || kin < 0 || kin >= m) return "selection map entry out of range";
    if (used[(size_t)k] == 2) return "selection map: more than two entries for one output bin";
    const int s = used[(size_t)k]++;
    if (kin >= nchan) continue;                    // a bin of the zero padding
    const int64_t red = (kin * half) % m;          // e^{-2 pi i k_in floor(m/2) / m}
    const double a = -2.0 * M_PI * (double)red / (double)m;
    const double sc = map_w[e] * scale;
    rs_in[(size_t)s * nout + k] = (int32_t)kin;
    rs_c[2 * ((size_t)s * nout + k)] = sc * std::cos(a);
    rs_c[2 * ((size_t)s * nout + k) + 1] = sc * std::sin(a);
  }
  for (int64_t q = 0; q < nout; ++q) {
    const double a = 2.0 * M_PI * (double)q / (double)nout;
    rtw[2 * q] = std::cos(a);
    rtw[2 * q + 1] = std::sin(a);
  }
  return nullptr;
}

// cpdelay.hip: its own builder, per window, with the terms compacted
struct HandCpdelay {
  std::vector<int32_t> rs_n, rs_k, rs_in;
  std::vector<double> rs_c, rtw;
};

const char* hand_cpdelay(int nwin, const double* wts, int64_t nres, int64_t m, int64_t nchan, double df, int64_t nmap, const int64_t* map_out,
                         const int64_t* map_in, const double* map_w, HandCpdelay& tr) {
  const int64_t nr = std::max<int64_t>(nres, 1);
  tr.rs_n.assign((size_t)nwin, 0);
  tr.rs_k.assign((size_t)nwin * nr, 0);
  tr.rs_in.assign((size_t)nwin * 2 * nr, -1);
  tr.rs_c.assign((size_t)nwin * 4 * nr, 0.0);
  tr.rtw.assign(2 * (size_t)nr, 0.0);
  if (nres > 0) {
    if (nmap < 1 || !map_out || !map_in || !map_w) return "the resampled spectra need the selection map";
    std::vector<int64_t> first((size_t)nres, -1), second((size_t)nres, -1);
    for (int64_t e = 0; e < nmap; ++e) {
      const int64_t k = map_out[e], kin = map_in[e];
      if (k < 0 || k >= nres || kin < 0 || kin >= m) return "selection map entry out of range";
      if (first[(size_t)k] < 0) first[(size_t)k] = e;
      else if (second[(size_t)k] < 0) second[(size_t)k] = e;
      else return "selection map: more than two entries for one output bin";
    }
    const int64_t half = m / 2;
    for (int w = 0; w < nwin; ++w) {
      int32_t n = 0;
      for (int64_t k = 0; k < nres; ++k) {
        int terms = 0;
        for (int64_t e : {first[(size_t)k], second[(size_t)k]}) {
          if (e < 0) continue;
          const int64_t kin = map_in[e];
          if (kin >= nchan || wts[(int64_t)w * nchan + kin] == 0.0) continue;     // a bin of the zero padding, or outside the window
          const double a = -2.0 * M_PI * (double)((kin * half) % m) / (double)m;  // e^{-2 pi i k_in floor(m/2) / m}
          const double sc = wts[(int64_t)w * nchan + kin] * map_w[e] * df;        // weight * (m df) * (1 / m)
          const size_t at = ((size_t)w * 2 + terms) * nr + n;
          tr.rs_in[at] = (int32_t)kin;
          tr.rs_c[2 * at] = sc * std::cos(a);
          tr.rs_c[2 * at + 1] = sc * std::sin(a);
          ++terms;
        }
        if (terms) tr.rs_k[(size_t)w * nr + n++] = (int32_t)k;
      }
      tr.rs_n[(size_t)w] = n;
    }
    for (int64_t q = 0; q < nres; ++q) {
      const double a = 2.0 * M_PI * (double)q / (double)nres;
      tr.rtw[2 * q] = std::cos(a);
      tr.rtw[2 * q + 1] = std::sin(a);
    }
  }
  return nullptr;
}

// runs.hip: the bins inside a window's support span, CSR
void hand_runs(int nwin, const double* win, int64_t nout, int64_t nchan, const std::vector<int32_t>& rs_in, std::vector<int32_t>& klist,
               std::vector<int32_t>& kofs) {
  klist.clear();
  kofs.assign((size_t)nwin + 1, 0);
  for (int w = 0; w < nwin; ++w) {
    int64_t lo = 0, hi = nchan;
    if (win) {
      lo = nchan;
      hi = 0;
      for (int64_t n = 0; n < nchan; ++n)
        if (win[w * nchan + n] != 0.0) { lo = std::min(lo, n); hi = n + 1; }
    }
    for (int64_t k = 0; k < nout; ++k)
      for (int sl = 0; sl < 2; ++sl) {
        const int32_t i = rs_in[(size_t)sl * nout + k];
        if (i >= lo && i < hi) { klist.push_back((int32_t)k); break; }
      }
    kofs[(size_t)w + 1] = (int32_t)klist.size();
  }
}

// cpft.hip: the bins fed by a nonzero channel, padded rows and counts
void hand_cpft(int nwin, const double* wts, int64_t nres, int64_t nchan, const std::vector<int32_t>& rs_in, std::vector<int32_t>& rs_n,
               std::vector<int32_t>& rs_k) {
  const int64_t nr = std::max<int64_t>(nres, 1);
  rs_n.assign((size_t)nwin, 0);
  rs_k.assign((size_t)nwin * nr, 0);
  for (int k = 0; k < nwin && nres > 0; ++k) {
    int32_t n = 0;
    for (int64_t q = 0; q < nres; ++q) {
      bool fed = false;
      for (int s = 0; s < 2; ++s) {
        const int32_t ch = rs_in[(size_t)s * nres + q];
        if (ch >= 0 && wts[(int64_t)k * nchan + ch] != 0.0) fed = true;
      }
      if (fed) rs_k[(size_t)k * nr + n++] = (int32_t)q;
    }
    rs_n[(size_t)k] = n;
  }
}

// ---- as the entries form their tables now ----

template <typename T>
bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// subband.hip, runs.hip, cpft.hip: (map_w * scale) (cos, sin)
std::vector<double> scaled(const ResampleTables& t, double scale) {
  std::vector<double> c(t.phase.size(), 0.0);
  for (size_t at = 0; at < t.in.size(); ++at) {
    if (t.in[at] < 0) continue;
    const double sc = t.w[at] * scale;
    c[2 * at] = sc * t.phase[2 * at];
    c[2 * at + 1] = sc * t.phase[2 * at + 1];
  }
  return c;
}

// padded rows and counts against a CSR pair
bool same_bins(int nwin, int64_t nr, const std::vector<int32_t>& rs_n, const std::vector<int32_t>& rs_k, const std::vector<int32_t>& ofs,
               const std::vector<int32_t>& list) {
  if (ofs.size() != (size_t)nwin + 1 || ofs[0] != 0 || (size_t)ofs[(size_t)nwin] != list.size()) return false;
  for (int w = 0; w < nwin; ++w) {
    if (ofs[(size_t)w + 1] - ofs[(size_t)w] != rs_n[(size_t)w]) return false;
    for (int32_t i = 0; i < rs_n[(size_t)w]; ++i)
      if (list[(size_t)ofs[(size_t)w] + i] != rs_k[(size_t)w * nr + i]) return false;
  }
  return true;
}

// one (case, window set, scale); win null: no windows (runs only)
bool check(const Map& M, int nwin, const double* win, double scale) {
  const int64_t nmap = (int64_t)M.mo.size(), nout = M.nout, nr = std::max<int64_t>(nout, 1);
  ResampleTables t;
  std::vector<int32_t> h_in, h_klist, h_kofs, ofs, list;
  std::vector<double> h_c, h_rtw;
  bool ok = resample_tables(nout, M.m, M.nchan, nmap, M.mo.data(), M.mi.data(), M.mw.data(), t) == nullptr;
  ok = ok && hand_tables(nout, M.m, M.nchan, scale, nmap, M.mo.data(), M.mi.data(), M.mw.data(), h_in, h_c, h_rtw) == nullptr;
  if (!ok) return false;
  ok = same_bits(t.in, h_in) && same_bits(scaled(t, scale), h_c) && same_bits(t.rtw, h_rtw);
  hand_runs(nwin, win, nout, M.nchan, h_in, h_klist, h_kofs);
  fed_bins(t, nout, nwin, M.nchan, win, Feeds::kSpan, ofs, list);
  ok = ok && same_bits(ofs, h_kofs) && same_bits(list, h_klist);
  if (!win) return ok;
  std::vector<int32_t> h_n, h_k;
  hand_cpft(nwin, win, nout, M.nchan, h_in, h_n, h_k);
  fed_bins(t, nout, nwin, M.nchan, win, Feeds::kNonzero, ofs, list);
  ok = ok && same_bins(nwin, nr, h_n, h_k, ofs, list);
  // cpdelay.hip: the window's weight folded in, the terms compacted
  HandCpdelay H;
  if (hand_cpdelay(nwin, win, nout, M.m, M.nchan, scale, nmap, M.mo.data(), M.mi.data(), M.mw.data(), H)) return false;
  std::vector<int32_t> rs_in((size_t)nwin * 2 * nr, -1);
  std::vector<double> rs_c((size_t)nwin * 4 * nr, 0.0);
  for (int w = 0; w < nwin; ++w)
    for (int32_t n = 0; n < ofs[(size_t)w + 1] - ofs[(size_t)w]; ++n) {
      const int64_t k = list[(size_t)ofs[(size_t)w] + n];
      int terms = 0;
      for (int sl = 0; sl < 2; ++sl) {
        const size_t e = (size_t)sl * nout + k;
        const int64_t kin = t.in[e];
        if (kin < 0 || win[(int64_t)w * M.nchan + kin] == 0.0) continue;
        const double sc = win[(int64_t)w * M.nchan + kin] * t.w[e] * scale;
        const size_t at = ((size_t)w * 2 + terms++) * nr + n;
        rs_in[at] = (int32_t)kin;
        rs_c[2 * at] = sc * t.phase[2 * e];
        rs_c[2 * at + 1] = sc * t.phase[2 * e + 1];
      }
    }
  return ok && same_bins(nwin, nr, H.rs_n, H.rs_k, ofs, list) && same_bits(rs_in, H.rs_in) && same_bits(rs_c, H.rs_c) && same_bits(t.rtw, H.rtw);
}

bool same_text(const char* a, const char* b) { return a && b && std::string(a) == b; }

int main() {
  std::vector<Map> maps;
  std::vector<std::vector<double>> xs;                // the series of the numeric cases, (re, im) per channel
@MAPS@
  long bad = 0, checked = 0;
  const size_t ncases = maps.size() - xs.size();
  for (size_t ci = 0; ci < ncases; ++ci) {
    const Map& M = maps[ci];
    const int64_t nc = M.nchan;
    // all ones; zero edges; one interior zero; all zero; a single nonzero channel
    std::vector<double> win(5 * (size_t)nc, 0.0);
    for (int64_t n = 0; n < nc; ++n) {
      win[n] = 1.0;
      win[nc + n] = (n == 0 || n == nc - 1) ? 0.0 : 0.5 + 0.25 * (double)(n % 3);
      win[2 * nc + n] = n == nc / 2 ? 0.0 : 1.0 + 0.125 * (double)(n % 5);
      win[4 * nc + n] = n == nc / 3 ? 0.75 : 0.0;
    }
    for (double scale : {@DF@, 0.37 / (double)M.m}) {
      for (int w = 0; w < 5; ++w) {
        if (!check(M, 1, win.data() + (size_t)w * nc, scale)) { std::printf("case %zu window set %d scale %g\n", ci, w, scale); ++bad; }
        ++checked;
      }
      if (!check(M, 5, win.data(), scale)) { std::printf("case %zu all five windows scale %g\n", ci, scale); ++bad; }
      if (!check(M, 1, nullptr, scale)) { std::printf("case %zu no windows scale %g\n", ci, scale); ++bad; }
      checked += 2;
    }
  }
  // nout < 1: one empty bin, no map needed
  {
    ResampleTables t;
    if (resample_tables(0, 8, 8, 0, nullptr, nullptr, nullptr, t) || t.in != std::vector<int32_t>{-1, -1} || t.rtw != std::vector<double>{0.0, 0.0}) ++bad;
    ++checked;
  }
  // the three refusals, word for word
  {
    ResampleTables t;
    HandCpdelay H;
    std::vector<int32_t> a;
    std::vector<double> b, c;
    const double one[4] = {1.0, 1.0, 1.0, 1.0};
    const int64_t mo3[3] = {1, 1, 1}, mi3[3] = {0, 1, 2}, mo_bad[1] = {4}, mi_bad[1] = {8};
    const char* e0 = resample_tables(4, 8, 4, 0, nullptr, nullptr, nullptr, t);
    if (!same_text(e0, hand_tables(4, 8, 4, 1.0, 0, nullptr, nullptr, nullptr, a, b, c)) ||
        !same_text(e0, hand_cpdelay(1, one, 4, 8, 4, 1.0, 0, nullptr, nullptr, nullptr, H)) ||
        !same_text(e0, "the resampled spectra need the selection map")) ++bad;
    for (int which = 0; which < 2; ++which) {
      const int64_t* mo = which ? mo_bad : mi3;       // an output bin of 4 (of 4), or an input bin of 8 (of 8)
      const int64_t* mi = which ? mi3 : mi_bad;
      const char* e1 = resample_tables(4, 8, 4, 1, mo, mi, one, t);
      if (!same_text(e1, hand_tables(4, 8, 4, 1.0, 1, mo, mi, one, a, b, c)) || !same_text(e1, hand_cpdelay(1, one, 4, 8, 4, 1.0, 1, mo, mi, one, H)) ||
          !same_text(e1, "selection map entry out of range")) ++bad;
    }
    const char* e2 = resample_tables(4, 8, 4, 3, mo3, mi3, one, t);
    if (!same_text(e2, hand_tables(4, 8, 4, 1.0, 3, mo3, mi3, one, a, b, c)) || !same_text(e2, hand_cpdelay(1, one, 4, 8, 4, 1.0, 3, mo3, mi3, one, H)) ||
        !same_text(e2, "selection map: more than two entries for one output bin")) ++bad;
    checked += 3;
  }
  // the snapshot tile as closure.hip, cpdelay.hip and runs.hip wrote it
  {
    constexpr int kMaxTile = 64, kTileLds = 65536;
    for (int64_t nt : {1, 3, 64, 65, 1000})
      for (int64_t n : {1, 8, 1024, 4096})
        for (int64_t row_bytes : {16 * (n + 1), 16 * n})
          for (int64_t tw_bytes : {(int64_t)0, 16 * std::max<int64_t>(n / 2, 1)}) {
            const int64_t tile = std::max<int64_t>(1, std::min<int64_t>({nt, (int64_t)kMaxTile, (kTileLds - tw_bytes) / row_bytes}));
            const int64_t lds = tile * row_bytes + tw_bytes;
            const int64_t ntiles = (nt + tile - 1) / tile;
            const SnapshotTile s = snapshot_tile(nt, row_bytes, tw_bytes);
            if (s.tile != tile || s.ntiles != ntiles || s.lds != lds) {
              std::printf("snapshot_tile(%lld, %lld, %lld): {%lld, %lld, %lld}, by hand {%lld, %lld, %lld}\n", (long long)nt, (long long)row_bytes,
                          (long long)tw_bytes, (long long)s.tile, (long long)s.ntiles, (long long)s.lds, (long long)tile, (long long)ntiles,
                          (long long)lds);
              ++bad;
            }
            ++checked;
          }
  }
  // the numeric cases: y[q] = sum_k Y[k] e^{+2 pi i k q / nout}, Y[k] = sum of x[in] (w df) e^{-2 pi i in floor(m/2) / m}, as the kernels sum
  for (size_t xi = 0; xi < xs.size(); ++xi) {
    const Map& M = maps[ncases + xi];
    const std::vector<double>& x = xs[xi];
    ResampleTables t;
    if (resample_tables(M.nout, M.m, M.nchan, (int64_t)M.mo.size(), M.mo.data(), M.mi.data(), M.mw.data(), t)) { ++bad; continue; }
    const std::vector<double> c = scaled(t, @DF@);
    std::vector<double> Y(2 * (size_t)M.nout, 0.0);
    for (int64_t k = 0; k < M.nout; ++k)
      for (int s = 0; s < 2; ++s) {
        const size_t at = (size_t)s * M.nout + k;
        if (t.in[at] < 0) continue;
        const double xr = x[2 * (size_t)t.in[at]], xim = x[2 * (size_t)t.in[at] + 1];
        Y[2 * k] += xr * c[2 * at] - xim * c[2 * at + 1];
        Y[2 * k + 1] += xr * c[2 * at + 1] + xim * c[2 * at];
      }
    for (int64_t q = 0; q < M.nout; ++q) {
      double yr = 0.0, yi = 0.0;
      for (int64_t k = 0; k < M.nout; ++k) {
        const double tr = t.rtw[2 * ((k * q) % M.nout)], ti = t.rtw[2 * ((k * q) % M.nout) + 1];
        yr += Y[2 * k] * tr - Y[2 * k + 1] * ti;
        yi += Y[2 * k] * ti + Y[2 * k + 1] * tr;
      }
      std::printf("y %zu %lld %.17g %.17g\n", xi, (long long)q, yr, yi);
    }
  }
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
'''


def _c_list(values, fmt):
    return '{' + ', '.join(fmt(v) for v in values) + '}'


def test_resample_plan_and_snapshot_tile_match_the_handwritten_loops(tmp_path):
    rng = NP.random.default_rng(20240607)
    lines, series = [], []
    for m, nout, nchan in CASES + NUMERIC:
        mo, mi, mw = dsp_readings.resample_map(m, nout)
        lines.append('  maps.push_back({%d, %d, %d, %s, %s, %s});' % (m, nout, nchan, _c_list(mo, lambda v: '%d' % v), _c_list(mi, lambda v: '%d' % v),
                                                                      _c_list(mw, lambda v: float(v).hex())))
    for m, nout, nchan in NUMERIC:
        x = rng.standard_normal(nchan) + 1j * rng.standard_normal(nchan)
        series.append(x)
        lines.append('  xs.push_back(%s);' % _c_list(x.view(NP.float64), lambda v: float(v).hex()))
    src = tmp_path / 'resample_check.cpp'
    src.write_text(RESAMPLE_PROGRAM.replace('@MAPS@', '\n'.join(lines)).replace('@DF@', float(DF).hex()))
    exe = tmp_path / 'resample_check'
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-I',
                           os.path.join(ROOT, 'prisim_amd', 'csrc_addon'), str(src), '-o', str(exe)])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    rows = out.strip().splitlines()
    # per case two scales of five single windows, the five together and none; one empty plan; three refusals; the tiles
    assert rows[-1] == 'checked %d bad 0' % (len(CASES) * 2 * 7 + 1 + 3 + 5 * 4 * 2 * 2), out
    # the spectrum formed from the tables against the reading of scipy.signal.resample: 1e-12 of df sum |x|
    for xi, ((m, nout, nchan), x) in enumerate(zip(NUMERIC, series)):
        got = NP.array([complex(float(r.split()[3]), float(r.split()[4])) for r in rows if r.startswith('y %d ' % xi)])
        assert got.shape == (nout,)
        want = dsp_readings.resample(m * DF * NP.fft.fftshift(NP.fft.ifft(x, m)), nout)
        err = NP.abs(got - want).max() / (DF * NP.abs(x).sum())
        print('resample (%d, %d, %d): %.3g of df sum |x|' % (m, nout, nchan, err))
        assert err <= 1e-12


# ---- the delay add-ons state their transform and resampling arithmetic once ----------------------------------------------------------

DELAY_ADDONS = ['csrc_subband/subband.hip', 'csrc_runs/runs.hip', 'csrc_closure/cpdelay.hip', 'csrc_closure/cpft.hip']


def test_delay_addons_take_their_arithmetic_from_delay_lines():
    """The sign of the shifted transform's operand and the direct sum's twiddle index are written in csrc_addon/delay_lines.h alone."""
    for rel in DELAY_ADDONS:
        with open(os.path.join(ROOT, 'prisim_amd', rel)) as f:
            txt = f.read()
        assert 'delay_lines.h"' in [ln.split('/')[-1] for ln in txt.splitlines() if ln.startswith('#include "')], rel
        assert 'rtw[' not in txt, rel
        assert '& 1)) ?' not in txt, rel
    with open(os.path.join(ROOT, 'prisim_amd', 'csrc_addon', 'delay_lines.h')) as f:
        txt = f.read()
    assert txt.count('rtw[') == 1 and txt.count('& 1)) ?') == 1
