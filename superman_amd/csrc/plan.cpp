// plan.cpp — the planner (pure host code, no HIP call): errors, matrix
// conversion, layouts, walk-column searches, make_plan, the segmented plan and
// its disk records, the plan cache, auto mode, plan fingerprints.  The device
// layer that walks a plan is engine.cpp, the schedulers schedule.cpp.
#include "engine.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>

#include <unistd.h>  // environ

namespace sup {

// ---------------------------------------------------------------- errors --
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }

bool env_on(const char* name, bool dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) != 0 : dflt;
}

// FNV-1a over bytes: the plan keys (seg_disk_key, plan_fingerprint) and the
// experiment-knob hash.
namespace {
struct Fnv1a {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t len) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < len; ++i) h = (h ^ c[i]) * 1099511628211ull;
  }
};

bool is_integral(const double* A, int n) {
  for (size_t i = 0; i < (size_t)n * n; ++i)
    if (A[i] != std::floor(A[i])) return false;
  return true;
}
}  // namespace

// -------------------------------------------------------------- matrices --
int to_double(const void* mat, sup_dtype t, int n, std::vector<double>& out) {
  if (!mat || n < 1 || n > SUP_MAX_N) {
    set_error("matrix pointer is null or n is outside [1, 64]");
    return SUP_EINVAL;
  }
  const size_t nn = (size_t)n * n;
  out.resize(nn);
  switch (t) {
    case SUP_INT32: {
      const int32_t* a = (const int32_t*)mat;
      for (size_t i = 0; i < nn; ++i) out[i] = (double)a[i];
      return SUP_OK;
    }
    case SUP_FLOAT32: {
      const float* a = (const float*)mat;
      for (size_t i = 0; i < nn; ++i) out[i] = (double)a[i];
      return SUP_OK;
    }
    case SUP_FLOAT64:
      std::memcpy(out.data(), mat, nn * sizeof(double));
      return SUP_OK;
  }
  set_error("unknown sup_dtype");
  return SUP_EINVAL;
}

void nw_start(const double* A, int n, double* x0, double* p0) {
  double p = 1.0;
  for (int j = 0; j < n; ++j) {
    double rs = 0.0;
    for (int k = 0; k < n; ++k) rs += A[(size_t)j * n + k];
    x0[j] = A[(size_t)j * n + (n - 1)] - rs / 2;
    p *= x0[j];
  }
  *p0 = p;
}

Layout default_layout(int n) {
  Layout l;
  const int nb = n - 1;
  l.L = nb < 6 ? nb : 6;
  const int rest = nb - l.L;
  // >= 2^10 walk steps per wave-chunk when possible, and at most 2^20
  // wave-chunks (8 MiB of partials) — fine-grained enough that the dynamic
  // chunk queue balances a whole MI355X (~5k resident waves) to < 1 %.
  // Small n (rest < 23): the walk shortens (down to 2^6 steps) until there are
  // 2^13 wave-chunks, so the whole chip walks instead of a few waves.
  int m = rest < 10 ? rest : 10;
  if (rest - m < 13) m = std::max(std::min(rest, 6), rest - 13);
  if (rest - 20 > m) m = rest - 20;
  if (m > 31) m = 31;  // 32-bit walk index in the kernels (n > 58 only)
  l.m = m;
  l.h = rest - m;
  return l;
}

Layout layout_with_walk(int n, int walk_log2) {
  Layout lay = default_layout(n);
  if (walk_log2 > 0) {
    const int rest = n - 1 - lay.L;
    lay.m = std::min(walk_log2, rest);
    lay.h = rest - lay.m;
    lay.fixed = true;
  }
  return lay;
}

// Walk-column order that keeps the row prefixes small: the first column is
// tried exhaustively, the rest is greedy (fewest newly covered rows, then
// fewest nonzeros, then lowest index); the order with the lowest prefix cost
// (VALU ops per Gray step, DESIGN.md §3.2: walk bit k flips with frequency
// 2^-(k+1) and costs 8*nblk adds, 8*nblk muls and one accumulate)
// wins.  Column n-1 (Nijenhuis-Wilf) is never a walk column.
std::vector<int> greedy_walk_order(const double* A, int n, int count) {
  const int nb = n - 1;
  count = std::min(count, nb);
  // column c's rows as a bit set (n <= 64): a candidate's new rows are one
  // popcount (the -o leaves plan a new matrix each: 0.3-0.7 ms -> ~0.05 ms)
  std::vector<uint64_t> cm(nb, 0);
  std::vector<int> nnz(n, 0);
  for (int c = 0; c < nb; ++c) {
    for (int i = 0; i < n; ++i)
      if (A[(size_t)i * n + c] != 0.0) cm[c] |= 1ull << i;
    nnz[c] = __builtin_popcountll(cm[c]);
  }
  auto greedy_from = [&](int first) {
    std::vector<int> order{first};
    std::vector<char> used(n, 0);
    used[first] = 1;
    uint64_t placed = cm[first];
    while ((int)order.size() < count) {
      int best = -1, bnew = 1 << 30;
      for (int c = 0; c < nb; ++c) {
        if (used[c]) continue;
        const int nw = __builtin_popcountll(cm[c] & ~placed);
        if (nw < bnew || (nw == bnew && nnz[c] < nnz[best])) best = c, bnew = nw;
      }
      used[best] = 1;
      order.push_back(best);
      placed |= cm[best];
    }
    return order;
  };
  // prefix_cost over the bit sets (the same row counts, so the same cost)
  auto cost_of = [&cm](const std::vector<int>& walk) {
    uint64_t placed = 0;
    double cost = 0.0, w = 0.5;
    for (int c : walk) {
      placed |= cm[c];
      cost += w * (16.0 * ((__builtin_popcountll(placed) + 7) / 8) + 1.0);
      w *= 0.5;
    }
    return cost;
  };
  std::vector<int> best;
  double bcost = 1e300;
  for (int f = 0; f < nb && count > 0; ++f) {
    std::vector<int> o = greedy_from(f);
    const double c = cost_of(o);
    if (c < bcost) bcost = c, best = o;
  }
  return best;
}

// ---- SkipPer column order (round 5) ----------------------------------------
// The SkipPer kernel's zero check at a wave-chunk's first state ends the chunk
// when a row that no walk and no lane column touches ("uniform tail" row) is
// exactly zero: its value is fixed for the whole chunk (x0 plus the chunk
// bits' columns).  Which rows those are is decided by the set of walk + lane
// columns, so the column map decides how many chunks SkipPer walks at all.
// SkipOrder's own map (identity) walks 25.7 % of config 5's states
// (profiles/r5); a map chosen for these chunk ends walks 10.6 % at a lower
// prefix cost (tools/probes/skip_sim.c).
namespace {
struct SkipOrderEval {
  const double* A;
  int n, m, L;
  std::vector<uint64_t> cm;  // column -> rows (bit set)
  std::vector<double> x0;
  // prefix-block cost of the first m columns (walk_cost's terms)
  double prefix_cost(const std::vector<int>& o) const {
    uint64_t placed = 0;
    double cost = 0.0, w = 0.5;
    for (int k = 0; k < m; ++k) {
      placed |= cm[o[k]];
      cost += w * (16.0 * ((__builtin_popcountll(placed) + 7) / 8) + 1.0);
      w *= 0.5;
    }
    return cost + w * 16.0 * ((n + 7) / 8);
  }
  // sampled fraction of wave-chunks whose first state has an exactly zero
  // uniform tail row (integer matrices: every sum here is exact); chunk
  // indices drawn as in seg_skip_estimate (jit.cpp)
  double kill(const std::vector<int>& o, int samples) const {
    const int nb = n - 1;
    uint64_t wl = 0;  // rows touched by a walk or lane column
    std::vector<char> used(nb, 0);
    for (int k = 0; k < m + L; ++k) wl |= cm[o[k]], used[o[k]] = 1;
    std::vector<int> high;
    for (int c = 0; c < nb; ++c)
      if (!used[c]) high.push_back(c);
    struct Row {
      double x0;
      std::vector<std::pair<int, double>> hi;
    };
    std::vector<Row> rows;
    for (int r = 0; r < n; ++r) {
      if ((wl >> r) & 1u) continue;
      Row q{x0[r], {}};
      for (int k = 0; k < (int)high.size(); ++k)
        if (A[(size_t)r * n + high[k]] != 0.0) q.hi.push_back({k, A[(size_t)r * n + high[k]]});
      rows.push_back(std::move(q));
    }
    if (rows.empty()) return 0.0;
    const int h = (int)high.size();
    int killed = 0;
    for (int s = 0; s < samples; ++s) {
      const uint64_t a = h ? ((uint64_t)s * 0x9E3779B97F4A7C15ull) >> (64 - std::min(h, 63)) : 0;
      const uint64_t g = a ^ (a >> 1);
      for (const Row& q : rows) {
        double v = q.x0;
        for (const auto& e : q.hi)
          if ((g >> e.first) & 1u) v += e.second;
        if (v == 0.0) {
          ++killed;
          break;
        }
      }
    }
    return (double)killed / samples;
  }
  double eff(const std::vector<int>& o, int samples) const { return prefix_cost(o) * (1.0 - kill(o, samples)); }
};
struct SplitMix64 {
  uint64_t z;
  uint64_t operator()() {
    uint64_t x = (z += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
  }
};
}  // namespace

// Walk + lane columns (m + L of them, walk first) for the SkipPer walk of an
// integer matrix, chosen on ops per nominal step x the fraction of chunks not
// ended at their first state; false when SkipOrder's own map (columns
// L..L+m-1 walk, 0..L-1 lanes) is not clearly worse (the estimate does not see
// the jumps inside a chunk, which favour SkipOrder's map: it must be beaten
// by 2x).  Deterministic (fixed seeds, results gathered in start order), so
// every process and host plans the same walk.  Random-restart local search:
// starts = the greedy prefix order, SkipOrder's map and random column sets;
// each start takes kRounds random moves (swap a walk or lane column with an
// unused one, or a walk with a lane column), keeping improvements on a
// 512-sample estimate; the best end on 8192 samples wins.
bool skip_walk_order(const double* A, int n, const Layout& lay, std::vector<int>& out,
                     const std::vector<int>* baseline, double factor) {
  const int nb = n - 1, m = lay.m, L = lay.L;
  if (m < 3 || m + L >= nb) return false;
  SkipOrderEval E{A, n, m, L, std::vector<uint64_t>(nb, 0), std::vector<double>(n)};
  for (int c = 0; c < nb; ++c)
    for (int i = 0; i < n; ++i)
      if (A[(size_t)i * n + c] != 0.0) E.cm[c] |= 1ull << i;
  double p0;
  nw_start(A, n, E.x0.data(), &p0);
  std::vector<int> ident;
  for (int k = 0; k < m; ++k) ident.push_back(L + k);
  for (int e = 0; e < L; ++e) ident.push_back(e);
  constexpr int kStarts = 16, kRounds = 1500, kScreen = 512, kFinal = 8192;
  std::vector<std::vector<int>> starts;
  {
    std::vector<int> g = greedy_walk_order(A, n, m + L);
    starts.push_back(g);
    starts.push_back(ident);
    SplitMix64 rnd{0x5EED5C1Bull};
    while ((int)starts.size() < kStarts) {
      std::vector<int> cols(nb);
      for (int c = 0; c < nb; ++c) cols[c] = c;
      for (int i = nb - 1; i > 0; --i) std::swap(cols[i], cols[rnd() % (uint64_t)(i + 1)]);
      cols.resize(m + L);
      starts.push_back(cols);
    }
  }
  std::vector<std::vector<int>> ends(starts.size());
  std::vector<double> effs(starts.size());
  auto search = [&](size_t si) {
    SplitMix64 rnd{0xC0FFEEull + 7919ull * si};
    std::vector<int> cur = starts[si];
    double cv = E.eff(cur, kScreen);
    std::vector<char> in(nb, 0);
    for (int c : cur) in[c] = 1;
    for (int it = 0; it < kRounds; ++it) {
      std::vector<int> t = cur;
      const int a = (int)(rnd() % (uint64_t)(m + L));
      // the other side of the move: an unused column, or (walk <-> lane) a
      // position on the other side
      const int n_out = nb - (m + L), n_other = a < m ? L : m;
      const int pick = (int)(rnd() % (uint64_t)(n_out + n_other));
      int incoming = -1;
      if (pick < n_out) {
        int k = pick;
        for (int c = 0; c < nb; ++c)
          if (!in[c] && k-- == 0) {
            incoming = c;
            break;
          }
        t[a] = incoming;
      } else {
        const int b = a < m ? m + (pick - n_out) : pick - n_out;
        std::swap(t[a], t[b]);
      }
      const double v = E.eff(t, kScreen);
      if (v < cv) {
        if (incoming >= 0) in[cur[a]] = 0, in[incoming] = 1;
        cur = std::move(t), cv = v;
      }
    }
    ends[si] = cur;
    effs[si] = E.eff(cur, kFinal);
  };
  {
    std::atomic<size_t> next{0};
    auto worker = [&]() {
      for (size_t i = next++; i < starts.size(); i = next++) search(i);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < std::min<int>(plan_threads(), (int)starts.size()); ++t) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
  }
  size_t bi = 0;
  for (size_t i = 1; i < ends.size(); ++i)
    if (effs[i] < effs[bi] - 1e-12) bi = i;
  const std::vector<int>& base = baseline && (int)baseline->size() == m + L ? *baseline : ident;
  const double e_base = E.eff(base, kFinal);
  if (std::getenv("SUP_JIT_VERBOSE"))
    std::fprintf(stderr, "chunk-end column search n=%d: best eff %.4f (cost %.3f, kill %.3f) vs the baseline's %.4f\n",
                 n, effs[bi], E.prefix_cost(ends[bi]), E.kill(ends[bi], kFinal), e_base);
  if (!(effs[bi] < factor * e_base)) return false;
  out = ends[bi];
  return true;
}

// A prefix-blocked plan of an integer matrix whose walk is predicted to take
// >= kChunkEndSearchSec (every state, walk_cost's ops): its walk + lane columns
// searched for chunk ends (skip_walk_order against its greedy order; taken when
// it cuts ops x chunks walked by 10 %).  Deterministic, from the matrix alone.
static constexpr double kChunkEndSearchSec = 4.0;
// fp64 VALU lane-ops per second of one MI355X on the walk kernels (measured:
// 46.6 ops/step at 7.98e11 steps/s on the n=40 bench), for the planners' time
// predictions (this search, SkipPer's, jit's auto mode).
static constexpr double kLaneOpsPerSec = 3.7e13;
// Predicted seconds of `steps` Gray steps at `ops` lane-ops each ((steps x ops)
// / rate, in this order: the predictions decide plans, and plans decide bits).
static double ops_seconds(double steps, double ops, double rate = kLaneOpsPerSec) { return steps * ops / rate; }
// Gray steps of an order-n walk on each of ndev devices.
static double gray_steps(int n, int ndev = 1) { return std::ldexp(1.0, n - 1) / std::max(ndev, 1); }

int improve_sparse_plan(const double* A, int n, const Layout& lay, Plan& P) {
  if (P.kind != kWalkSparse || !P.integral || lay.m < 3 ||
      ops_seconds(gray_steps(n), walk_cost(P)) < kChunkEndSearchSec)
    return SUP_OK;
  std::vector<int> base;
  for (int k = 0; k < lay.m; ++k) base.push_back(P.colmap[lay.L + k]);
  for (int e = 0; e < lay.L; ++e) base.push_back(P.colmap[e]);
  SegChoice c;
  if (!skip_walk_order(A, n, lay, c.order, &base, 0.9)) return SUP_OK;
  Plan Q;
  const int rc = make_plan(A, n, kWalkSparse, false, lay, Q, &c);
  if (rc == SUP_OK) P = std::move(Q);
  return rc;
}

double walk_cost(const Plan& P) {
  if (P.kind == kWalkDense) return 2.0 * P.n + 1.0;
  if (P.kind == kWalkSeg) return seg_walk_cost(P);
  double cost = 0.0, w = 0.5;
  for (int k = 0; k < P.lay.m; ++k, w *= 0.5) cost += w * (16.0 * P.nblk[P.lay.L + k] + 1.0);
  return cost + w * 16.0 * ((P.n + 7) / 8);  // tail: the rest of the walk bits, bounded
}

// ops per nominal Gray step, chunks the walk skips discounted: what the
// planner compares walks on (the reported cost model stays per walked step)
static double walk_cost_eff(const Plan& P) {
  return P.kind == kWalkSeg ? walk_cost(P) * (1.0 - P.seg_skip) : walk_cost(P);
}

double walk_seconds(const Plan& P, double steps) { return ops_seconds(steps, walk_cost_eff(P)); }

// SUP_NO_CHUNK_ENDS=1 (experiments, A/B): no chunk ends in the prefix-blocked
// and exact walks (walk_sparse.hip); the sums are the same, the ended chunks'
// terms being exact zeros.
static bool no_chunk_ends() { static const bool off = env_on("SUP_NO_CHUNK_ENDS", false); return off; }  // read once

int make_plan(const double* A, int n, WalkKind kind, bool identity_map, const Layout& lay, Plan& P,
              const SegChoice* choice) {
  if (n < 1 || n > SUP_MAX_N) {
    set_error("n must be in [1, 64]");
    return SUP_EINVAL;
  }
  P = Plan();
  P.n = n;
  P.NP = pad8(n);
  P.kind = kind;
  P.lay = lay;
  P.integral = is_integral(A, n);
  const int nb = n - 1;  // flippable columns (column n-1 is the Nijenhuis-Wilf column)
  const int L = lay.L, m = lay.m;

  // ---- engine bit -> matrix column
  P.colmap.resize(nb);
  for (int e = 0; e < nb; ++e) P.colmap[e] = e;
  // a caller-chosen walk + lane order: a map searched for chunk ends
  // (skip_walk_order: SkipPer, and long prefix-blocked / exact / double-double
  // walks of integer matrices), or the exact walk's greedy order (exact.cpp)
  const bool given_order = (kind == kWalkSkip || kind == kWalkDense || kind == kWalkSparse) && choice && m > 0;
  if (!identity_map && (kind == kWalkSparse || kind == kWalkSeg || given_order) && m > 0) {
    // walk bits get the greedy prefix order (greedy_walk_order; the segmented
    // walk: seg_walk_order), lane bits the next L columns of that order, high
    // bits the rest in matrix order.
    int segb = 0;
    std::vector<int> order;
    // a recorded order (plan choices on disk) is taken only when it is a set of
    // m + L distinct flippable columns: a corrupted or foreign record would
    // index past the matrix or give a column map that is not a permutation
    auto valid_order = [&](const std::vector<int>& o) {
      if ((int)o.size() != m + L) return false;
      std::vector<char> seen(nb, 0);
      for (int v : o) {
        if (v < 0 || v >= nb || seen[v]) return false;
        seen[v] = 1;
      }
      return true;
    };
    if (given_order) {
      if (!valid_order(choice->order)) {
        set_error("walk column order: not m + L distinct flippable columns");
        return SUP_EINVAL;
      }
      order = choice->order;
    } else if (kind == kWalkSeg && choice && valid_order(choice->order) && choice->b >= 0 && choice->b <= m) {
      order = choice->order;
      segb = choice->b;
    } else {
      order = kind == kWalkSeg ? seg_walk_order(A, n, m, m + L, &segb, lay.cc_cap) : greedy_walk_order(A, n, m + L);
    }
    P.seg_b = segb;
    if (kind == kWalkSeg) P.seg_order.assign(order.begin(), order.begin() + (m + L));
    std::vector<char> used(n, 0);
    for (int k = 0; k < m; ++k) P.colmap[L + k] = order[k], used[order[k]] = 1;
    for (int e = 0; e < L; ++e) P.colmap[e] = order[m + e], used[order[m + e]] = 1;
    int e = L + m;
    // High bits (the wave-chunk index).  The segmented walk on an integer
    // matrix skips the wave-chunks whose rows untouched by the walk columns are
    // exactly zero in every lane; a high column with no nonzero in those rows
    // never changes that, so those columns take the top bits: contiguous
    // shards (sup_perman_shard, -p5) then see the same skip pattern.  (Config
    // 5 before: the top chunk bit alone decided skipping, half the shards had
    // nothing to walk at 2, 4 and 8 GPUs.)  Otherwise matrix order.
    std::vector<char> top(n, 0);
    if (kind == kWalkSeg || given_order) {
      // (SkipPer ends a chunk on a row no walk and no lane column touches)
      std::vector<char> wrow(n, 0);
      for (int k = 0; k < (given_order ? m + L : m); ++k)
        for (int i = 0; i < n; ++i) wrow[i] |= A[(size_t)i * n + order[k]] != 0.0;
      for (int c = 0; c < nb && P.integral; ++c) {
        top[c] = 1;
        for (int i = 0; i < n; ++i)
          if (!wrow[i] && A[(size_t)i * n + c] != 0.0) top[c] = 0;
      }
    }
    for (int pass = 0; pass < 2; ++pass)
      for (int c = 0; c < nb; ++c)
        if (!used[c] && top[c] == pass) P.colmap[e++] = c;
  }

  // ---- engine row order
  P.rowperm.resize(n);
  for (int j = 0; j < n; ++j) P.rowperm[j] = j;
  P.nblk.assign(std::max(nb, 1), 0);
  P.rowmask.assign(n, 0);
  if (kind != kWalkDense) {
    // rows in first-touch order over the walk columns (walk order), then the rest
    std::vector<char> placed(n, 0);
    std::vector<int> order;
    order.reserve(n);
    for (int k = 0; k < m; ++k) {
      const int c = P.colmap[L + k];
      for (int i = 0; i < n; ++i)
        if (!placed[i] && A[(size_t)i * n + c] != 0.0) {
          placed[i] = 1;
          order.push_back(i);
        }
      P.nblk[L + k] = ((int)order.size() + 7) / 8;
    }
    for (int i = 0; i < n; ++i)
      if (!placed[i]) order.push_back(i);
    P.rowperm = order;
    if (kind == kWalkSeg) {  // segment 0 sub-ordered (jit.cpp)
      std::vector<int> walk(m);
      for (int k = 0; k < m; ++k) walk[k] = P.colmap[L + k];
      P.rowperm = seg_row_order(A, n, walk);
    }
    // a walk column may touch no new row: nblk must still cover its own rows,
    // which are all inside the prefix, so the prefix count above is correct.
  }
  for (int e = 0; e < nb; ++e)
    if (e < L || e >= L + m) P.nblk[e] = (n + 7) / 8;  // not used by the walk; keep sane

  // ---- tables
  P.cols.assign((size_t)2 * std::max(nb, 1) * P.NP, 0.0);
  for (int e = 0; e < nb; ++e) {
    const int c = P.colmap[e];
    for (int j = 0; j < n; ++j) {
      const double v = A[(size_t)P.rowperm[j] * n + c];
      P.cols[(size_t)(2 * e) * P.NP + j] = v;
      P.cols[(size_t)(2 * e + 1) * P.NP + j] = -v;
    }
  }
  std::vector<double> x0(n);
  double p0;
  nw_start(A, n, x0.data(), &p0);
  P.x0.assign(P.NP, 0.0);
  for (int j = 0; j < n; ++j) P.x0[j] = x0[P.rowperm[j]];

  // ---- skipper metadata
  P.umask = 0;
  for (int j = 0; j < n; ++j) {
    const int i = P.rowperm[j];
    bool lane_touched = false;
    for (int e = 0; e < L; ++e)
      if (A[(size_t)i * n + P.colmap[e]] != 0.0) lane_touched = true;
    if (!lane_touched) P.umask |= 1ull << j;
    uint64_t rm = 0;
    for (int k = 0; k < m; ++k)
      if (A[(size_t)i * n + P.colmap[L + k]] != 0.0) rm |= 1ull << k;
    P.rowmask[j] = rm;
    // a lane-uniform row no walk column touches is constant over a wave-chunk:
    // exactly zero at the chunk's first state, the chunk ends there (walk_sparse)
    if ((kind == kWalkSparse || kind == kWalkDense) && !lane_touched && rm == 0 && !no_chunk_ends())
      P.chunk_ends |= 1ull << j;
  }
  if (kind == kWalkSeg) return build_seg(P, choice ? choice->budget : 0, choice ? choice->hi : 0);
  return SUP_OK;
}

// Auto mode's bar where nothing bounds the saving (orders below
// kJitWarmMinN; jit != 0 never asks): no walk that short repays a plan.
static constexpr double kJitMinSavingSec = 3.0;
// Auto mode (jit = 0) decides once per matrix and request, and every later
// run follows that decision (AutoRecord): the plan (walk-order search +
// compiles, seg_cold_predict: ~1.6 s at n = 40 on a GPU box, cold) is paid
// once, the walk time it saves on every run.  So a plan is started when the
// walk time it can save over kAutoRuns runs would repay it — the bench
// matrix, a 0.5 s saving per run on one MI355X, specialises on a fresh host;
// a matrix walked once loses at most the plan's cost.  Once the search and
// the compiler check have run their cost is spent, and the segmented walk is
// taken when it saves kJitWarmSavingSec per run.
static constexpr double kAutoRuns = 4.0;
// When an earlier process recorded this matrix's segmented-walk choices (disk
// cache, make_seg_plan), the plan is rebuilt in ~5-50 ms and its code object
// loads from disk: auto mode specialises whenever the walk saves more than this.
static constexpr double kJitWarmSavingSec = 0.1;
// Below this order no walk lasts kJitWarmSavingSec (2^29 steps at ~3e12/s):
// auto mode does not look at the disk cache.
static constexpr int kJitWarmMinN = 30;

static int plan_for_uncached(const double* A, int n, sup_kernel kernel, const Layout& lay, Plan& P, int jit,
                             int ndev, int dev, double min_saving);
static double auto_min_saving(const double* A, int n, const Layout& lay, int jit);

// Chunk start of the segmented walk (start index's column sums, row copies,
// trees of every cached state), in VALU ops per lane: ~750 fitted from config
// 3's kernel time against its walk length, ~1700 from the d = 0.2 companion's
// (profiles/r2/probe_walklen.log).
static constexpr double kSegStartOps = 2048.0;

// The segmented walk on the default layout, or on longer wave-chunks where its
// steps are cheap: a chunk's walk (2^m steps) should be >= 32 chunk starts.
// Both walks are planned and the one with fewer ops per nominal step, chunk
// start and chunk skip included, wins.  At least 2^14 chunks remain (8 per
// resident wave of one GPU, one per wave of each of 8 GPUs).  Round 6 lowered
// this from 2^15: config 2 (n = 32) then walks m = 11 instead of 10, 0.555
// against 0.580 ms (chunk starts 13.5 -> 10.2 % of the wave cycles, queue tail
// 3.4 -> 7 %; profiles/r6/cfg2_knobs.log), config 3 m = 15 instead of 14
// (1.905 against 1.92-1.94 ms, profiles/r6/cfg3_m.log).  The layout depends
// only on the matrix, so every GPU count sums the same chunks (bit-identical
// results).
static constexpr int kSegMinChunkBits = 14;

// Hash of every SUP_JIT_* variable that shapes a plan or its generated source
// (experiment knobs), so a process that changes one gets a fresh plan; the
// cache location, source dumps and log verbosity do not change a plan.
static uint64_t knob_hash() {
  Fnv1a f;
  for (char** e = environ; e && *e; ++e) {
    const char* v = *e;
    if (std::strncmp(v, "SUP_JIT_", 8) != 0 || !std::strncmp(v, "SUP_JIT_CACHE_DIR=", 18) ||
        !std::strncmp(v, "SUP_JIT_DUMP=", 13) || !std::strncmp(v, "SUP_JIT_VERBOSE=", 16) ||
        !std::strncmp(v, "SUP_JIT_COLD_RATIO=", 19))
      continue;
    f.bytes(v, std::strlen(v));
    f.bytes("\xff", 1);
  }
  return f.h;
}

// Disk key of a segmented-walk plan: what its choices depend on, the layout
// request, experiment knobs and the toolchain the choices were priced with.
// For a non-integer matrix the choices (walk-order search, trees, budget, the
// generated source) depend on the zero pattern only, so the key is the
// pattern: matrices that differ only in their nonzero values (a rescaled row,
// another draw of the same pattern) share one record and one kernel.  Integer
// matrices add their values (the chunk-skip estimate and the column order of
// the chunk bits look at exact zeros of row sums).
static uint64_t seg_disk_key(const double* A, int n, const Layout& lay) {
  Fnv1a f{0x5eed5e9a11ull ^ jit_toolchain_hash()};
  const size_t nn = (size_t)n * n;
  const bool integral = is_integral(A, n);
  const int32_t head[] = {7 /* format: bump when the planner changes */, n, lay.L, lay.m, (int32_t)lay.fixed, (int32_t)integral};
  f.bytes(head, sizeof head);
  if (integral) {
    f.bytes(A, nn * sizeof(double));
  } else {
    std::vector<unsigned char> pat((nn + 7) / 8, 0);
    for (size_t i = 0; i < nn; ++i)
      if (A[i] != 0.0) pat[i / 8] |= (unsigned char)(1u << (i % 8));
    f.bytes(pat.data(), pat.size());
  }
  const uint64_t k = knob_hash();
  f.bytes(&k, sizeof k);
  return f.h;
}

static int make_seg_plan(const double* A, int n, const Layout& lay, Plan& P) {
  // a later process rebuilds the plan from its recorded choices (no search,
  // no compiler check: ~0.1 s instead of seconds)
  const uint64_t dkey = seg_disk_key(A, n, lay);
  {
    int m2 = 0;
    SegChoice c;
    if (seg_choice_load(dkey, &m2, &c) && m2 >= 3 && m2 <= lay.m + lay.h && (!lay.fixed || m2 == lay.m)) {
      Layout l2 = lay;
      l2.m = m2;
      l2.h = lay.m + lay.h - m2;
      l2.cc_cap = c.cc_cap;
      if (make_plan(A, n, kWalkSeg, false, l2, P, &c) == SUP_OK) return SUP_OK;
    }
  }
  const auto t_cold = std::chrono::steady_clock::now();
  // a short walk whose 4-cached-bit kernel touches scratch in its loop
  // (build_seg's check) is planned again with 3 cached bits
  auto plan = [A, n](const Layout& l, Plan& Q) {
    int r = make_plan(A, n, kWalkSeg, false, l, Q);
    if (r == SUP_OK && Q.seg_loop_scratch && l.cc_cap > 3) {
      Layout l3 = l;
      l3.cc_cap = 3;
      r = make_plan(A, n, kWalkSeg, false, l3, Q);
    }
    return r;
  };
  int rc = plan(lay, P);
  if (rc) return rc;
  if (!lay.fixed) {
    const int mmax = std::min(lay.m + lay.h - kSegMinChunkBits, 31);
    int m2 = lay.m;
    while (m2 < mmax && std::ldexp(P.seg_model_ops, m2) < 32.0 * kSegStartOps) ++m2;
    if (m2 != lay.m) {
      Layout l2 = lay;
      l2.m = m2;
      l2.h = lay.m + lay.h - m2;
      Plan s2;
      if (plan(l2, s2) == SUP_OK) {
        auto eff = [](const Plan& q) {
          return (1.0 - q.seg_skip) * (q.seg_model_ops + std::ldexp(kSegStartOps, -q.lay.m));
        };
        if (eff(s2) < eff(P)) P = std::move(s2);
      }
    }
  }
  SegChoice c;
  c.order = P.seg_order;
  c.b = P.seg_b;
  c.budget = P.seg_budget;
  c.hi = P.seg_hi;
  c.cc_cap = P.lay.cc_cap;
  seg_choice_store(dkey, P.lay.m, c);
  // what this cold plan cost (search + the compiler check's compiles): auto
  // mode's cold bar on this host (plan_for)
  const double cold_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_cold).count();
  seg_cost_store(n, cold_s);
  if (std::getenv("SUP_JIT_VERBOSE"))
    std::fprintf(stderr, "cold segmented plan n=%d: %.3f s (compiles %.3f s wall on this thread)\n", n, cold_s,
                 jit_compile_ms_thread() * 1e-3);
  return SUP_OK;
}

// Plans are pure functions of (matrix, request, layout): repeated calls on the
// same matrix (the bench's steps, a shard per rank, -p6 items, reductions
// revisiting a leaf) reuse the plan instead of re-running the walk-order
// search (~5-15 ms at n = 40, comparable to an 8-GPU shard's walk).
namespace {
struct PlanKey {
  uint64_t hash;
  int n, kernel, L, m, jit, ndev;
  bool fixed;      // walk length asked for (sup_opts::walk_log2): make_seg_plan keeps it
  uint64_t knobs;  // SUP_JIT_* experiment settings the planner and code generator read
  // Not in the key: auto mode's bar (auto_min_saving), which moves with the
  // disk cache (this matrix's choices recorded, this host's cold plan cost) —
  // possibly written meanwhile by another rank or thread.  The first auto-mode
  // decision for a matrix and request is kept for the process, so a call after
  // sup_prepare / sup_plan_key (the bench's plan-agreement check) walks the
  // plan that was checked.
  bool operator<(const PlanKey& o) const {
    return std::tie(hash, n, kernel, L, m, jit, ndev, fixed, knobs) <
           std::tie(o.hash, o.n, o.kernel, o.L, o.m, o.jit, o.ndev, o.fixed, o.knobs);
  }
};
std::mutex g_plan_mu;
// cached plans are shared, not copied: a cached call takes a reference (the
// segmented plan's source, tables and trees are ~200 KB at n = 40)
std::map<PlanKey, std::pair<std::vector<double>, std::shared_ptr<const Plan>>> g_plans;
constexpr size_t kPlanCacheMax = 32;
}  // namespace

int plan_for_shared(const double* A, int n, sup_kernel kernel, const Layout& lay, std::shared_ptr<const Plan>& out,
                    int jit, int ndev, int dev, bool keep) {
  const size_t nn = (size_t)n * n;
  // in-process cache key only (the entry also keeps the matrix and compares
  // it): four independent FNV-style lanes, so the multiply chain is a quarter
  // as long (n = 32: 1.7 -> ~0.5 us per call)
  uint64_t l[4] = {1469598103934665603ull, 0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull};
  size_t i = 0;
  for (; i + 4 <= nn; i += 4)
    for (int k = 0; k < 4; ++k) {
      uint64_t b;
      std::memcpy(&b, A + i + k, 8);
      l[k] = (l[k] ^ b) * 1099511628211ull;
    }
  for (; i < nn; ++i) {
    uint64_t b;
    std::memcpy(&b, A + i, 8);
    l[0] = (l[0] ^ b) * 1099511628211ull;
  }
  uint64_t h = l[0];
  for (int k = 1; k < 4; ++k) h = (h ^ l[k]) * 1099511628211ull;
  // ndev only feeds auto mode's compile-or-not decision
  const PlanKey key{h, n, (int)kernel, lay.L, lay.m, jit, jit == 0 ? ndev : 0, lay.fixed, knob_hash()};
  auto cached = [&]() {  // under g_plan_mu
    auto it = g_plans.find(key);
    if (it == g_plans.end() || !std::equal(A, A + nn, it->second.first.begin())) return false;
    out = it->second.second;
    return true;
  };
  {
    std::lock_guard<std::mutex> g(g_plan_mu);
    if (cached()) return SUP_OK;
  }
  auto P = std::make_shared<Plan>();
  const int rc = plan_for_uncached(A, n, kernel, lay, *P, jit, ndev, dev, auto_min_saving(A, n, lay, jit));
  if (rc) return rc;
  if (!keep) {  // a plan walked once (a batch's leaf): the cache keeps the caller's plans
    out = P;
    return SUP_OK;
  }
  std::lock_guard<std::mutex> g(g_plan_mu);
  if (cached()) return SUP_OK;  // another thread planned the same request meanwhile: its plan stands
  if (g_plans.size() >= kPlanCacheMax) g_plans.clear();
  static uint64_t next_uid = 0;
  P->uid = ++next_uid;
  out = P;
  g_plans[key] = {std::vector<double>(A, A + nn), out};
  return SUP_OK;
}

int plan_for(const double* A, int n, sup_kernel kernel, const Layout& lay, Plan& P, int jit, int ndev, int dev) {
  std::shared_ptr<const Plan> sp;
  const int rc = plan_for_shared(A, n, kernel, lay, sp, jit, ndev, dev);
  if (rc == SUP_OK) P = *sp;
  return rc;
}

// SkipPer evaluates only the states its zero checks cannot rule out; its
// checks and jumps cost it efficiency per evaluated state.  Round 5's kernel
// (segment-start checks, walk_sparse's paired steps elsewhere) with the
// searched column map (skip_walk_order) on config 5 int: 19.3 modelled ops per
// visited state, 10.6 % visited, 0.779 s — 2.31e13 ops/s against the plain
// walks' 3.7e13 (profiles/r5/probe_skip_searched_map.log; SkipOrder's map:
// 0.69, round 4's per-state kernel: 0.37).  Round 6's kernel forms
// (walk_skip.hip: straight-line segments) walk the same states in 0.537 s,
// 3.35e13 ops/s: 0.90 — the price SkipPer is weighed at; the column search's
// threshold below keeps round 5's rate, so the plans (and bits) it picks are
// unchanged.
static constexpr double kSkipEfficiency = 0.62;
static constexpr double kSkipPriceEfficiency = 0.90;
// SkipPer walks predicted (every state, SkipOrder's map, at kSkipEfficiency)
// to take at least this long search their column map for chunk ends
// (~0.2-0.6 s of host time; config 5: 9.5 s predicted, 0.54 s walked after
// the search).
static constexpr double kSkipSearchMinSec = 4.0;

// Fraction of the states the SkipPer plan P evaluates, measured on a fixed
// sample of its wave-chunks (8 evenly spaced ranges, ~1/64 of the walk) on
// device `dev`; -1 without a device.  Deterministic: visited counts depend only
// on the matrix and the chunks, not on timing.
static double skip_visited_fraction(const Plan& P, int dev) {
  int nd = 0;
  if (device_count(&nd) != SUP_OK || nd < 1) return -1.0;
  if (dev < 0 || dev >= nd) dev = 0;
  const uint64_t C = P.lay.chunks(), len = std::max<uint64_t>(1, C / 512);
  uint64_t vis = 0, tot = 0;
  for (uint64_t i = 0; i < 8; ++i) {
    uint64_t c0 = (2 * i + 1) * C / 16;
    if (c0 + len > C) c0 = C - len;
    RangeResult r;
    if (run_range(dev, P, c0, c0 + len, true, r) != SUP_OK) return -1.0;
    vis += r.visited;
    tot += len << (P.lay.L + P.lay.m);
  }
  return tot ? (double)vis / (double)tot : 1.0;
}

// Auto mode's bar for starting a segmented plan: the walk time it can save
// per run must exceed the predicted cold plan cost (seg_cold_predict: n, this
// host's plan threads and its recorded speed) over kAutoRuns runs; ~0 (the
// warm bar) when an earlier process left this matrix's plan choices and
// kernel in the disk cache.
static double auto_min_saving(const double* A, int n, const Layout& lay, int jit) {
  if (jit != 0 || n < kJitWarmMinN) return kJitMinSavingSec;  // below: no walk lasts even the lowest bar
  if (seg_choice_exists(seg_disk_key(A, n, lay))) return kJitWarmSavingSec;
  return std::max(kJitWarmSavingSec, seg_cold_predict(n) / kAutoRuns);
}

// Auto mode's first decision per matrix and request, on disk (round 4).  The
// bar above moves with the cache: a cold run keeps the ahead-of-time walk
// where the search + compile would cost more than they save, and once a plan's
// choices are recorded (a --jit 1 run, another rank) the same command would
// specialise — a different operation order, so different last bits of an fp64
// result between two runs of one command.  So auto mode records what it
// decided the first time and later processes follow it (cold and warm runs
// print the same bits; --jit 1 / -1 pick a walk explicitly).  Recorded only
// where the decision can depend on the cache: auto mode (jit = 0) and a walk
// long enough to save the warm bar (n >= 37 dense: the -o leaves never write).
struct AutoRecord {
  uint64_t key = 0;
  int recorded = -1;  // -1: none (or not recordable), 0 / 1 as recorded
  bool active = false;
  AutoRecord(const double* A, int n, const Layout& lay, sup_kernel kernel, int ndev, int jit, double walk_s) {
    active = jit == 0 && n >= kJitWarmMinN && walk_s >= kJitWarmSavingSec;
    if (!active) return;
    key = seg_disk_key(A, n, lay) ^ (0x9e3779b97f4a7c15ull * (uint64_t)(1 + (int)kernel)) ^
          ((uint64_t)std::max(ndev, 1) << 48);
    recorded = auto_decision_load(key);
  }
  // records seg unless a decision is on disk; returns the decision to follow
  // (another process that decided first wins)
  bool store(bool seg) const {
    if (active && recorded < 0) return auto_decision_store(key, seg ? 1 : 0) == 1;
    return seg;
  }
};

static int plan_for_uncached(const double* A, int n, sup_kernel kernel, const Layout& lay, Plan& P, int jit,
                             int ndev, int dev, double min_saving) {
  // candidates in preference order; the cheapest by walk_cost wins
  std::vector<WalkKind> kinds;
  auto make_seg = [&](Plan& s) { return make_seg_plan(A, n, lay, s); };
  switch (kernel) {
    case SUP_KERNEL_SKIPPER: {
      // SkipPer only gains where some x_j(S) is exactly zero.  With a
      // non-integer entry that is a measure-zero coincidence, so SkipPer
      // evaluates every state; with integer entries the fraction it
      // evaluates is measured on a sample of its chunks (GPU; without a
      // device the request keeps SkipPer).  The segmented walk (same sum,
      // every state) runs instead when that is cheaper.
      int rc = make_plan(A, n, kWalkSkip, false, lay, P);
      if (rc) return rc;
      const bool integral = P.integral;
      // an integer matrix whose SkipPer walk is long: the column map chosen
      // for the chunks SkipPer ends at their first state (skip_walk_order;
      // decided from the matrix alone, so every device count and host plans
      // the same walk)
      if (integral && n >= 10 &&
          ops_seconds(gray_steps(n), walk_cost(P), kSkipEfficiency * kLaneOpsPerSec) >= kSkipSearchMinSec) {
        SegChoice c;
        Plan Q;
        if (skip_walk_order(A, n, lay, c.order, nullptr, 0.5) && make_plan(A, n, kWalkSkip, false, lay, Q, &c) == SUP_OK)
          P = std::move(Q);
      }
      if (jit < 0 || n < 10 || lay.m < 3) return SUP_OK;
      const double steps = gray_steps(n, ndev);
      double skip_cost = walk_cost(P) / (integral ? kSkipPriceEfficiency : 1.0);  // f <= 1
      const AutoRecord rec(A, n, lay, kernel, ndev, jit, ops_seconds(steps, skip_cost));
      if (rec.recorded == 0) return SUP_OK;
      Plan s;
      if (rec.recorded == 1) {  // the recorded decision: the segmented walk (choices on disk)
        if (make_seg(s) == SUP_OK) P = std::move(s);
        return SUP_OK;
      }
      auto decide = [&]() -> bool {
        // auto mode: no segmented plan (its search takes ~0.1-1 s) where even a
        // free walk could not save the compile
        if (jit < 1 && ops_seconds(steps, skip_cost) < min_saving) return false;
        if (make_seg(s) != SUP_OK) return false;
        if (walk_cost_eff(s) >= skip_cost) return false;
        // the plan is paid for now: the segmented walk when it saves the warm bar
        const double bar = std::min(min_saving, kJitWarmSavingSec);
        if (jit < 1 && ops_seconds(steps, skip_cost - walk_cost_eff(s)) < bar) return false;
        if (integral) {
          const double f = skip_visited_fraction(P, dev);
          if (f < 0.0) return false;
          skip_cost *= f;
        }
        const double saved = ops_seconds(steps, skip_cost - walk_cost_eff(s));
        return walk_cost_eff(s) < skip_cost && (jit >= 1 || saved >= bar);
      };
      const bool seg = decide();
      if (rec.store(seg)) {
        if (seg) P = std::move(s);
        else if (make_seg(s) == SUP_OK) P = std::move(s);  // another process decided first
      }
      return SUP_OK;
    }
    case SUP_KERNEL_DENSE_PLAIN: return make_plan(A, n, kWalkDense, false, lay, P);
    case SUP_KERNEL_DENSE_LDS: {
      int rc = make_plan(A, n, kWalkDense, false, lay, P);
      P.lds = true;
      return rc;
    }
    case SUP_KERNEL_SEGMENTED:
      if (n < 10 || lay.m < 3) {
        set_error("the segmented walk needs n >= 10 (>= 3 walk bits)");
        return SUP_EUNSUPPORTED;
      }
      return make_seg(P);
    case SUP_KERNEL_SPARYSER: kinds = {kWalkSparse}; break;
    case SUP_KERNEL_DENSE: kinds = {kWalkDense}; if (n >= 8) kinds.push_back(kWalkSparse); break;
    default: set_error("unknown sup_kernel"); return SUP_EINVAL;
  }
  Plan best;
  int rc = make_plan(A, n, kinds[0], false, lay, best);
  if (rc == SUP_OK && kinds[0] == kWalkSparse) rc = improve_sparse_plan(A, n, lay, best);
  if (rc) return rc;
  for (size_t i = 1; i < kinds.size(); ++i) {
    Plan c;
    if (make_plan(A, n, kinds[i], false, lay, c) == SUP_OK && walk_cost(c) < walk_cost(best) &&
        (kinds[i] != kWalkSparse || improve_sparse_plan(A, n, lay, c) == SUP_OK))
      best = std::move(c);
  }
  const double best_s = ops_seconds(gray_steps(n, ndev), walk_cost(best));
  const bool may_save = best_s >= min_saving;  // auto mode: skip the segmented plan's search where it cannot pay
  if (jit >= 0 && n >= 8 && lay.m >= 3) {
    const AutoRecord rec(A, n, lay, kernel, ndev, jit, best_s);
    Plan s;
    if (rec.recorded == 1) {  // the recorded decision: the segmented walk (choices on disk)
      if (make_seg(s) == SUP_OK) best = std::move(s);
    } else if (rec.recorded < 0 && (jit >= 1 || may_save)) {
      bool seg = false;
      const bool planned = make_seg(s) == SUP_OK;
      if (planned && walk_cost_eff(s) < walk_cost(best)) {
        // the search and the compiler check are paid now: the segmented walk
        // when it saves the warm bar per run
        const double saved = ops_seconds(gray_steps(n, ndev), walk_cost(best) - walk_cost_eff(s));
        seg = jit >= 1 || saved >= std::min(min_saving, kJitWarmSavingSec);
      }
      if (rec.store(seg) && planned) best = std::move(s);
    } else if (rec.recorded < 0) {
      if (rec.store(false) && make_seg(s) == SUP_OK) best = std::move(s);  // another process decided first
    }
  }
  P = std::move(best);
  return SUP_OK;
}

uint64_t plan_fingerprint(const Plan& P) {
  // everything that decides which wave-chunk sums which subsets, in what
  // order and with which operations: walk kind, layout, column map, the
  // signed column table, the segmented walk's choices and its kernel source
  Fnv1a f;
  const int32_t head[] = {P.n, (int32_t)P.kind, (int32_t)P.lds, P.lay.L, P.lay.m, P.lay.h, P.seg_cc, P.seg_b,
                          P.seg_budget, P.seg_kp};
  f.bytes(head, sizeof head);
  f.bytes(P.colmap.data(), P.colmap.size() * sizeof(int));
  f.bytes(P.cols.data(), P.cols.size() * sizeof(double));
  f.bytes(P.x0.data(), P.x0.size() * sizeof(double));
  f.bytes(&P.jit_key, sizeof P.jit_key);
  f.bytes(P.jtab.data(), P.jtab.size() * sizeof(double));
  return f.h;
}

double pairwise_host(const std::vector<double>& v) {
  if (v.empty()) return 0.0;
  size_t p = 1;
  while (p < v.size()) p <<= 1;
  std::vector<double> a(p, 0.0);
  std::copy(v.begin(), v.end(), a.begin());
  while (p > 1) {
    p >>= 1;
    for (size_t i = 0; i < p; ++i) a[i] = a[2 * i] + a[2 * i + 1];
  }
  return a[0];
}

}  // namespace sup
