// wk_ctc_beam.hip -- CTC prefix beam search (N-best decode) on [B][T][V] fp32
// log-probs, blank = 0.  The algorithm is the one include/wakeword.h and
// tests/ctc_beam_ref.py state: per frame the K best non-blank tokens C_t, every
// live prefix stays and is extended by every token of C_t, an extension that is
// itself a live prefix adds to that prefix's stay, the W largest totals survive.
//
// Two launches on the caller's stream, no host synchronisation, no atomics:
//   cand    one wave per (b, t) row.  The row is read once, 16 bytes per lane
//           where it is 16-byte aligned (RowSplit, wk_ctc_lattice_dev.h).  The
//           K best (value, id) pairs so far live one per lane, sorted; an
//           element enters only if it beats the K-th (value greater, or equal
//           with the lower id: compares only),
//           which a wave-wide ballot decides for 256 elements at a time, so the
//           common chunk costs one max and one compare per lane.  An insertion
//           is a lane shift (DPP) of the pairs behind it.  The wave writes C_t
//           in selection order to d_cand, and, sorted by id, with the values
//           and the blank's, to the workspace.
//   recur   one wave per utterance, one lane per beam slot, sequential over
//           frames.  A lane holds its prefix as a node of the search tree: node
//           id t W + slot + 1 of the frame and slot that made it (0: the empty
//           prefix), the parent's id, the last token, the length and a hash of
//           the prefix and of its parent's.  Per frame:
//             merge   an extension (i, c) is the live prefix j iff j's last
//                     token is c and j's parent prefix is i's prefix.  The same
//                     parent node proves it.  A prefix can leave the beam and
//                     be made again later as another node, so where the hashes
//                     and lengths agree but the nodes differ, the two chains are
//                     walked up the node table until they meet (equal) or a
//                     token differs: identity is by prefix, exactly, and the
//                     hash only keeps the walk rare;
//             select  each lane keeps the best of its stay and its K
//                     extensions (registers); W rounds of a wave maximum pick
//                     the winner (a stay before an extension, then the lower
//                     lane, then the lower token: candidate order), hand it to
//                     lane r and rescan the winner's lane;
//             store   a lane whose new prefix is an extension writes the node
//                     (parent id, token): one row of up to W words per frame.
//           After the last frame lane i < n_best walks its chain up the table
//           into d_tokens.
// (+) is lse2 (wk_ctc_lattice_dev.h); every sum has one fixed order, so equal
// inputs give equal bits.
#include <math.h>

#include "wakeword.h"
#include "wk_ctc_lattice_dev.h"

namespace wk {
namespace {

constexpr int kCtcBeamMaxBeam = 64;          // one lane per slot
constexpr int kCtcBeamMaxTopK = 32;          // one register per extension
constexpr int kNoId = 0x7FFFFFFF;            // an empty entry of the candidate list: loses to every id

struct CtcBeamWs {
  int64_t* nodes;    // [batch][T * W + 1]: node id -> parent id << 16 | token (id 0, the empty prefix, has no word)
  int32_t* cid;      // [batch][T][K] C_t sorted by id, -1 beyond min(K, V-1) entries
  float* cval;       // [batch][T][K] their log-probs
  float* blank;      // [batch][T]    lp[b, t, 0]
  int64_t bytes;
};

CtcBeamWs ctc_beam_layout(void* base, int64_t batch, int32_t T, int32_t beam, int32_t top_k) {
  CtcBeamWs w;
  const int64_t frames = batch * T;
  w.nodes = (int64_t*)base;
  w.cid = (int32_t*)(w.nodes + frames * beam + batch);
  w.cval = (float*)(w.cid + frames * top_k);
  w.blank = w.cval + frames * top_k;
  w.bytes = round_up_256(8 * (frames * beam + batch) + 4 * (2 * frames * top_k + frames));
  return w;
}

// (v, id) ranks before (w, jd): the greater value, or an equal one with the lower id.
__device__ __forceinline__ bool beats(float v, int id, float w, int jd) { return v > w || (v == w && id < jd); }

// ---- candidate selection ------------------------------------------------------------
struct TopList {
  float kv;      // lane i: the i-th best pair so far
  int kid;
  float tv;      // the K-th best: what an element has to beat
  int tid;
};

// Offers each lane's (v, id) to the list, one insertion per pass of the loop.
__device__ __forceinline__ void offer(TopList& s, float v, int id, bool valid, int K, int lane) {
  bool pend = valid && beats(v, id, s.tv, s.tid);
  uint64_t m;
  while ((m = __ballot(pend)) != 0) {
    const int l = __builtin_ctzll(m);
    const float xv = read_lane(v, l);
    const int xid = read_lane(id, l);
    const float pv = prev_lane(0.0f, s.kv);
    const int pid = prev_lane(0, s.kid);
    if (beats(xv, xid, s.kv, s.kid)) {                           // x goes in front of this lane's pair:
      const bool behind = lane > 0 && beats(xv, xid, pv, pid);   // ... and of the previous lane's, which moves here
      s.kv = behind ? pv : xv;
      s.kid = behind ? pid : xid;
    }
    s.tv = read_lane(s.kv, K - 1);
    s.tid = read_lane(s.kid, K - 1);
    pend = pend && lane != l && beats(v, id, s.tv, s.tid);
  }
}

__global__ __launch_bounds__(256) void ctc_beam_cand_kernel(const float* __restrict__ lp, const int32_t* __restrict__ in_len,
                                                            int64_t rows, int T, int V, int K, CtcBeamWs w,
                                                            int32_t* __restrict__ cand_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= rows) return;                                   // (wave-uniform)
  const int b = (int)(row / T), t = (int)(row % T);
  const int Tb = in_len ? min(max(in_len[b], 0), T) : T;
  if (t >= Tb) {
    if (cand_out && lane < K) cand_out[row * K + lane] = -1;
    return;
  }
  const float* p = lp + row * V;
  TopList s = {neg_inf(), kNoId, neg_inf(), kNoId};
  const RowSplit r = row_split(p, V);
  const int head = r.head, nq = r.nq, tail0 = r.tail0;
  if (head) {
    const bool in = lane < head;
    offer(s, p[min(lane, head - 1)], lane, in && lane != 0, K, lane);
  }
  // Quads: a lane past the last one re-reads the last (an address inside the row; `in` keeps it out of the ranking).
  const float4* q4 = r.q4;
  if (nq > 0) {
    float4 cur = q4[min(lane, nq - 1)];
    for (int base = 0; base < nq; base += 64) {
      const int q = base + lane;
      const float4 nxt = q4[min(q + 64, nq - 1)];            // the next chunk is in flight while this one is ranked
      const bool in = q < nq;
      const int id0 = head + 4 * q;
      // one compare per lane decides the common chunk: nothing in it reaches the K-th best
      const float m4 = fmaxf(fmaxf(cur.x, cur.y), fmaxf(cur.z, cur.w));
      if (__ballot(in && m4 >= s.tv) != 0) {
        offer(s, cur.x, id0, in && id0 != 0, K, lane);
        offer(s, cur.y, id0 + 1, in, K, lane);
        offer(s, cur.z, id0 + 2, in, K, lane);
        offer(s, cur.w, id0 + 3, in, K, lane);
      }
      cur = nxt;
    }
  }
  if (tail0 < V) {
    const int id = tail0 + lane;
    const bool in = id < V;
    offer(s, p[min(id, V - 1)], id, in && id != 0, K, lane);
  }
  // lanes 0 .. nv-1 hold C_t in selection order; the workspace takes it sorted by id
  const bool have = lane < K && s.kid != kNoId;
  int pos = 0;
  for (int j = 0; j < K; ++j) pos += read_lane(s.kid, j) < s.kid;
  if (!have) pos = lane;                                    // (the empty entries stay behind the nv valid ones)
  if (lane < K) {
    if (cand_out) cand_out[row * K + lane] = have ? s.kid : -1;
    w.cid[row * K + pos] = have ? s.kid : -1;
    w.cval[row * K + pos] = have ? s.kv : neg_inf();
  }
  if (lane == 0) w.blank[row] = p[0];
}

// ---- beam recurrence ----------------------------------------------------------------
constexpr uint32_t kHashRoot = 0x811C9DC5u;
__device__ __forceinline__ uint32_t hash_next(uint32_t h, int token) {
  h = (h ^ (uint32_t)(token + 1)) * 0x01000193u;
  return h ^ (h >> 15);
}

// Whether nodes x and y, both at depth `depth`, spell the same prefix.
__device__ __forceinline__ bool same_prefix(const int64_t* nodes, int64_t x, int64_t y, int depth) {
  for (int s = 0; s < depth && x != y; ++s) {
    const int64_t ex = nodes[x], ey = nodes[y];
    if ((ex & 0xFFFF) != (ey & 0xFFFF)) return false;
    x = ex >> 16;
    y = ey >> 16;
  }
  return x == y;
}

template <int KMAX>
__global__ __launch_bounds__(64) void ctc_beam_recur_kernel(const float* __restrict__ lp, const int32_t* __restrict__ in_len, int T,
                                                            int V, int W, int K, int n_best, int max_len, CtcBeamWs w,
                                                            int32_t* __restrict__ tokens, int32_t* __restrict__ lengths,
                                                            float* __restrict__ scores) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = __builtin_amdgcn_readfirstlane(in_len ? min(max(in_len[b], 0), T) : T);
  const int64_t frame0 = (int64_t)b * T;
  int64_t* nodes = w.nodes + frame0 * W + b;

  // lane s < nlive: hypothesis s
  int nlive = 1;
  float pb = lane == 0 ? 0.0f : neg_inf(), pnb = neg_inf(), p = pb;
  int e = -1, len = 0;                  // last token (-1: none), length
  int64_t node = 0, par = -1;
  uint32_t h = kHashRoot, ph = 0;

  // lane k: candidate k of the frame, ascending id; loaded a frame ahead (they do not depend on the beam)
  int cidr = -1, cid_next = -1;
  float cvalr = neg_inf(), cval_next = neg_inf(), lp0 = 0.0f, lp0_next = 0.0f;
  if (Tb > 0) {
    cid_next = lane < K ? w.cid[frame0 * K + lane] : -1;
    cval_next = lane < K ? w.cval[frame0 * K + lane] : neg_inf();
    lp0_next = w.blank[frame0];
  }

  for (int t = 0; t < Tb; ++t) {
    const int64_t fr = frame0 + t;
    const bool live = lane < nlive;
    const float lpe_row = lp[fr * V + max(e, 0)];                    // lp[e]: used after the merge, so its latency hides behind it
    cidr = cid_next, cvalr = cval_next, lp0 = lp0_next;
    if (t + 1 < Tb) {
      cid_next = lane < K ? w.cid[(fr + 1) * K + lane] : -1;
      cval_next = lane < K ? w.cval[(fr + 1) * K + lane] : neg_inf();
      lp0_next = w.blank[fr + 1];
    }

    // where this lane's last token stands in C_t (-1: not in it); lanes k >= K hold id -1, which no token equals
    const int e_or_none = e > 0 ? e : -2;
    int kpos = -1;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) kpos = read_lane(cidr, k) == e_or_none ? k : kpos;

    // merge: lane j finds the live i whose extension by e_j is j's prefix
    float merge_from = neg_inf();       // the mass lane j's prefix takes from the extension that equals it, before lp[e]
    uint32_t merged = 0;                // bit k: this lane's extension by candidate k is a live prefix
    for (int i = 0; i < nlive; ++i) {
      const uint32_t hi = read_lane(h, i);
      const int leni = read_lane(len, i), ei = read_lane(e, i);
      const int64_t nodei = read_lane(node, i);
      const float pbi = read_lane(pb, i), pi = read_lane(p, i);
      bool hit = live && kpos >= 0 && len == leni + 1 && ph == hi;
      if (__ballot(hit && par != nodei) != 0) {                      // (rare: the parent prefix was made twice, or the hashes collide)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");      // other lanes' node words
        if (hit && par != nodei) hit = same_prefix(nodes, par, nodei, leni);
      }
      uint64_t m = __ballot(hit);
      if (m != 0) {
        if (hit) merge_from = e == ei ? pbi : pi;
        do {
          const int j = __builtin_ctzll(m);
          const int kb = read_lane(kpos, j);
          if (lane == i) merged |= 1u << kb;
          m &= m - 1;
        } while (m != 0);
      }
    }

    // candidates: this lane's stay and its K extensions
    float spb = neg_inf(), spnb = neg_inf(), stot = neg_inf();
    if (live) {
      const float lpe = len > 0 ? lpe_row : neg_inf();
      spb = lp0 + p;
      spnb = lse2(lpe + pnb, lpe + merge_from);
      stot = lse2(spb, spnb);
    }
    float ext[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {      // (k >= K: id -1, value -inf)
      const int ck = read_lane(cidr, k);
      const float cv = read_lane(cvalr, k);
      ext[k] = live && ck > 0 && !((merged >> k) & 1u) ? cv + (ck == e ? pb : p) : neg_inf();
    }
    float best = stot;
    int bk = -1;                        // -1: the stay
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (ext[k] > best) best = ext[k], bk = k;

    // select: round r fills slot r
    float n_pb = neg_inf(), n_pnb = neg_inf(), n_p = neg_inf();
    int n_e = -1, n_len = 0;
    int64_t n_node = 0, n_par = -1;
    uint32_t n_h = kHashRoot, n_ph = 0;
    bool made = false;
    int cnt = 0;
    for (int r = 0; r < W; ++r) {
      const float wmax = wave_max(best);
      if (!(wmax > neg_inf())) break;
      const uint64_t ma = __ballot(best == wmax), ms = __ballot(best == wmax && bk < 0);
      if (ma == 0) break;
      const int win = __builtin_ctzll(ms != 0 ? ms : ma);
      const int kw = read_lane(bk, win);
      const int64_t nodew = read_lane(node, win);
      const uint32_t hw = read_lane(h, win);
      const int lenw = read_lane(len, win);
      if (kw < 0) {
        const float a = read_lane(spb, win), c = read_lane(spnb, win);
        const int ew = read_lane(e, win);
        const int64_t parw = read_lane(par, win);
        const uint32_t phw = read_lane(ph, win);
        if (lane == r) n_pb = a, n_pnb = c, n_p = wmax, n_e = ew, n_len = lenw, n_node = nodew, n_par = parw, n_h = hw, n_ph = phw;
      } else {
        const int tok = read_lane(cidr, kw);
        if (lane == r) {
          n_pb = neg_inf(), n_pnb = wmax, n_p = wmax, n_e = tok, n_len = lenw + 1;
          n_node = (int64_t)t * W + r + 1, n_par = nodew, n_h = hash_next(hw, tok), n_ph = hw;
          made = true;
        }
      }
      // the winner leaves its lane's candidates; the lane's best is found again
      const int gone = lane == win ? kw : -2;      // per lane, so the loop below is selects, not a branch per k
      stot = gone == -1 ? neg_inf() : stot;
      best = stot, bk = -1;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        ext[k] = k == gone ? neg_inf() : ext[k];
        const bool up = ext[k] > best;
        best = up ? ext[k] : best;
        bk = up ? k : bk;
      }
      ++cnt;
    }
    nlive = cnt;
    pb = n_pb, pnb = n_pnb, p = n_p, e = n_e, len = n_len, node = n_node, par = n_par, h = n_h, ph = n_ph;
    if (made) nodes[node] = (par << 16) | (int64_t)e;
  }

  // results: slot i is hypothesis i
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const int64_t out0 = (int64_t)b * n_best;
  if (lane < n_best) {
    lengths[out0 + lane] = lane < nlive ? len : -1;
    scores[out0 + lane] = lane < nlive ? p : neg_inf();
  }
  for (int i = 0; i < n_best; ++i) {                     // -1 beyond each length
    const int li = i < nlive ? min(read_lane(len, i), max_len) : 0;
    int32_t* row = tokens + (out0 + i) * max_len;
    for (int x = li + lane; x < max_len; x += 64) row[x] = -1;
  }
  if (lane < n_best && lane < nlive) {
    int32_t* row = tokens + (out0 + lane) * max_len;
    int64_t id = node;
    for (int s = len - 1; s >= 0 && id > 0; --s) {
      const int64_t word = nodes[id];
      if (s < max_len) row[s] = (int32_t)(word & 0xFFFF);
      id = word >> 16;
    }
  }
}

template <int KMAX>
void launch_recur(const float* lp, const int32_t* in_len, int64_t batch, int T, int V, int W, int K, int n_best, int max_len,
                  const CtcBeamWs& w, int32_t* tokens, int32_t* lengths, float* scores, hipStream_t st) {
  hipLaunchKernelGGL(ctc_beam_recur_kernel<KMAX>, dim3((unsigned)batch), dim3(64), 0, st, lp, in_len, T, V, W, K, n_best, max_len, w,
                     tokens, lengths, scores);
}

}  // namespace
}  // namespace wk

using wk::invalid;

extern "C" {

int64_t wk_ctc_beam_workspace_bytes(int64_t batch, int32_t T, int32_t beam, int32_t top_k) {
  if (batch <= 0 || T <= 0 || beam < 1 || beam > wk::kCtcBeamMaxBeam || top_k < 1 || top_k > wk::kCtcBeamMaxTopK ||
      batch > wk::kCtcMaxFrames || batch * T > wk::kCtcMaxFrames)
    return 0;
  return wk::ctc_beam_layout(nullptr, batch, T, beam, top_k).bytes;
}

wk_status wk_ctc_beam(const float* d_log_probs, int64_t batch, int32_t T, int32_t vocab, const int32_t* d_input_lengths_or_null,
                      int32_t beam, int32_t top_k, int32_t n_best, int32_t max_len, void* d_workspace, int32_t* d_tokens,
                      int32_t* d_lengths, float* d_scores, int32_t* d_cand_or_null, int32_t device, void* stream) {
  if (!d_log_probs || !d_workspace || !d_tokens || !d_lengths || !d_scores) return invalid("wk_ctc_beam: null pointer");
  if (batch <= 0 || T <= 0) return invalid("wk_ctc_beam: batch and T must be positive");
  if (vocab < 2 || vocab > wk::kCtcMaxVocab) return invalid("wk_ctc_beam: vocab must be in [2, 65536]");
  if (beam < 1 || beam > wk::kCtcBeamMaxBeam) return invalid("wk_ctc_beam: beam must be in [1, 64]");
  if (top_k < 1 || top_k > wk::kCtcBeamMaxTopK) return invalid("wk_ctc_beam: top_k must be in [1, 32]");
  if (n_best < 1 || n_best > beam) return invalid("wk_ctc_beam: n_best must be in [1, beam]");
  if (max_len < 1) return invalid("wk_ctc_beam: max_len < 1");
  if (batch > wk::kCtcMaxFrames || batch * T > wk::kCtcMaxFrames) return invalid("wk_ctc_beam: batch * T > 2^28");
  if ((uintptr_t)d_workspace & 15) return invalid("wk_ctc_beam: d_workspace must be 16-byte aligned");
  if (device < 0) return invalid("wk_ctc_beam: device < 0");
  const wk::CtcBeamWs w = wk::ctc_beam_layout(d_workspace, batch, T, beam, top_k);
  hipStream_t st = (hipStream_t)stream;
  return wk::on_device(device, [&]() -> wk_status {
    const int64_t rows = batch * T;
    hipLaunchKernelGGL(wk::ctc_beam_cand_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, d_log_probs,
                       d_input_lengths_or_null, rows, T, vocab, top_k, w, d_cand_or_null);
    if (top_k <= 8)
      wk::launch_recur<8>(d_log_probs, d_input_lengths_or_null, batch, T, vocab, beam, top_k, n_best, max_len, w, d_tokens,
                          d_lengths, d_scores, st);
    else if (top_k <= 16)
      wk::launch_recur<16>(d_log_probs, d_input_lengths_or_null, batch, T, vocab, beam, top_k, n_best, max_len, w, d_tokens,
                           d_lengths, d_scores, st);
    else
      wk::launch_recur<32>(d_log_probs, d_input_lengths_or_null, batch, T, vocab, beam, top_k, n_best, max_len, w, d_tokens,
                           d_lengths, d_scores, st);
    return wk::ctc_launched("wk_ctc_beam");
  });
}

}  // extern "C"
