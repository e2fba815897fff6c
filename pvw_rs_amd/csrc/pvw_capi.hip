// pvw_capi.hip -- C ABI (include/pvw_hip.h) over the gfx950 kernels: context, parameter
// arithmetic, device residency of A-hat / B-hat, encrypt / decrypt orchestration, decode.
//
// The product path has no CPU fallback: every bulk polynomial operation runs in a HIP
// kernel and every device entry point fails with PVW_ERR_INTERNAL when no gfx950 device
// is usable.  Host-side code here is what the reference also does on the host with
// num-bigint: parameter set-up (src/params/parameters.rs:117-195), the f64 correctness
// gate (:510-551) and the integer gadget decode (src/crypto/decryption.rs:10-247).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pvw_hip.h"
#include "pvw_arith.h"
#include "pvw_bignum.h"
#include "pvw_chacha.h"
#include "pvw_decode.h"
#include "pvw_kernels.h"
#include "pvw_shamir_fields.h"
#if PVW_TUNING
#include "../../include/pvw_hip_tuning.h"
#endif
#include "pvw_ahead_ring.h"

using namespace pvw;

// ------------------------------------------------------------------------ errors
static thread_local std::string g_last_error;

static int32_t fail(int32_t code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
#define PVW_HIP_AS(code, expr)                                                             \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(code, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); \
  } while (0)
#define PVW_HIP(expr) PVW_HIP_AS(PVW_ERR_INTERNAL, expr)
#define PVW_TRY(expr)              \
  do {                             \
    int32_t rc_ = (expr);          \
    if (rc_ != PVW_OK) return rc_; \
  } while (0)

// a stream under capture takes no allocation and no wait
static bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
  (void)hipGetLastError();
  return capturing;
}

// ------------------------------------------------------------------------ number theory (host)
static bool is_prime_u64(u64 n) {
  if (n < 2) return false;
  static const u64 small[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
  for (u64 p : small)
    if (n % p == 0) return n == p;
  u64 d = n - 1;
  int s = 0;
  while ((d & 1) == 0) { d >>= 1; ++s; }
  for (u64 a : small) {
    u128 x = 1, b = a % n;
    for (u64 e = d; e; e >>= 1) {
      if (e & 1) x = x * b % n;
      b = b * b % n;
    }
    if (x == 1 || x == n - 1) continue;
    bool comp = true;
    for (int i = 1; i < s; ++i) {
      x = x * x % n;
      if (x == n - 1) { comp = false; break; }
    }
    if (comp) return false;
  }
  return true;
}
static u32 ilog2(u32 x) { u32 b = 0; while ((1u << b) < x) ++b; return b; }

// smallest primitive `order`-th root of unity mod q: this build's deterministic psi
static u64 min_primitive_root(const Mod& m, u32 order) {
  u64 e = (m.q - 1) / order, w = 0;
  for (u64 g = 2;; ++g) {
    w = powmod(g, e, m);
    if (powmod(w, order / 2, m) == m.q - 1) break;
  }
  u64 best = w, cur = w, w2 = mulmod(w, w, m);
  for (u32 i = 1; i < order / 2; ++i) {
    cur = mulmod(cur, w2, m);
    if (cur < best) best = cur;
  }
  return best;
}
// runtime-l host NTT (table building, gadget): natural in, bit-reversed out
static void host_ntt_forward(u64* a, u32 l, const u64* tw, const Mod& m) {
  u32 step = l;
  for (u32 mm = 1; mm < l; mm <<= 1) {
    step >>= 1;
    for (u32 i = 0; i < mm; ++i) {
      u64 w = tw[mm + i];
      for (u32 j = 2 * i * step; j < 2 * i * step + step; ++j) {
        u64 u = a[j], v = mulmod(a[j + step], w, m);
        a[j] = addmod(u, v, m.q);
        a[j + step] = submod(u, v, m.q);
      }
    }
  }
}

// ------------------------------------------------------------------------ context
struct ProfRec {
  std::string name;
  hipEvent_t a, b;
};
struct Workspace {
  hipStream_t stream = nullptr;
  bool own_stream = false;
  u64* rhat = nullptr;       // [L][k][l]  (x4: up to four r-hat / s-hat vectors)
  size_t rhat_bytes = 0;
  i64* esmall = nullptr;     // [rowsA + rowsB][l] sampled e1 | e2 coefficients of one encrypt (compact addends, l <= 16)
  u64* dpart = nullptr;      // range sums of a split decrypt_mac [nsplit][dealers][L][l]
  size_t dpart_bytes = 0;
  u64* sumbuf = nullptr;     // ciphertext sums (sum_layout): slice sums | summed c1 | summed c2 rows | noisy | results
  size_t sumbuf_bytes = 0;
  u64* scalars = nullptr;    // [n]
  u64* c1 = nullptr;         // [rowsA][L][l]
  u64* c2 = nullptr;         // [rowsB][L][l]
  void* scratch = nullptr;   // growable staging
  size_t scratch_bytes = 0;
  // digit-GEMM operands for up to 16 vectors (allocated on first use)
  u64* vhat16 = nullptr;     // [16][L][k][l]
  signed char* yd = nullptr; // vector digit tiles
  int* sy = nullptr;         // their column sums
  u64* gtmpA = nullptr;      // GEMM intermediates [limb][slot][v][row]
  u64* gtmpB = nullptr;
  u64* gtmpK = nullptr;      // ... for key generation (k rows)
  u64* shares = nullptr;     // Shamir shares of one pass of dealers [SHARE_PASS][n] (pvw_deal_shares*; built with the digit buffers)
  size_t shares_bytes = 0;
  u64* interp = nullptr;     // checked reconstruction: points | products | weight matrix (shamir_interp_words; grown by the call)
  size_t interp_bytes = 0;
  u64* interp_wide = nullptr;   // the same over a prime below 2^256 (shamir_interp_wide_words)
  size_t interp_wide_bytes = 0;
  u64* packw = nullptr;      // packed dealing: Lw | zt | w | 1/j! (shamir_packed_words; public, grown by the call)
  size_t packw_bytes = 0;
  u64* packw_wide = nullptr; // the same over a prime below 2^256 (shamir_packed_wide_words; public, grown by the call)
  size_t packw_wide_bytes = 0;
  u64* handover_wide = nullptr;  // wide handover: points | column weights | a group's scale, Cauchy entries, coin | column map
  size_t handover_wide_bytes = 0;   // (shamir_handover_wide_words; public, grown by the call)
  u64* handover_io = nullptr;    // wide handover on device pointers: weight rows (public) | the digit report [P][R] (HandoverIo; secret)
  size_t handover_io_bytes = 0;
  u64* handover = nullptr;       // one-word handover weights: points | column weights | a group's targets, scale, Cauchy entries, coin
  size_t handover_bytes = 0;     // (shamir_handover_words; public, grown by the call)
  u64* handover_rows = nullptr;  // one-word handover on device pointers: the weight rows [T][D] (public)
  size_t handover_rows_bytes = 0;
  u64* correct = nullptr;    // corrected reconstruction: M | public matrices | syndromes | locators (CorrectLayout; grown by the call)
  size_t correct_bytes = 0;
  u64* correct_wide = nullptr;   // the same over a prime below 2^256 (CorrectLayout<WideField>)
  size_t correct_wide_bytes = 0;
  // helper stream + events (ws_aux): decode of chunk i under the MAC of chunk i+1, key uploads under key generation
  hipStream_t aux = nullptr;
  bool aux_used = false;     // by the current host call: drained by host_call
  std::vector<hipEvent_t> events;
  // seed-mode encrypts on a busy stream (encrypt_enqueue's ahead path): 2R sets of (r-hat [L][k][l] | e_small) that the prologue
  // fills on `aux` while the caller's stream still runs earlier work; which set a call takes and when a guard is due:
  // pvw_ahead_ring.h.  Allocated by the first such call (ahead_sets).
  AheadRing ahead;
  char* ahead_block = nullptr;
  size_t ahead_set_bytes = 0, ahead_rhat_bytes = 0;
  std::vector<hipEvent_t> ahead_done;   // per set: recorded on `aux` behind the prologue that fills it
  hipEvent_t ahead_guard[2] = {nullptr, nullptr};   // per bank: recorded on the caller's stream behind the MAC that reads its last set
  hipEvent_t ahead_mark = nullptr;      // recorded behind the MAC of a call that could have gone ahead and did not record a guard
  hipEvent_t ahead_last = nullptr;      // the guard or mark behind the latest such MAC: not complete = that MAC is still outstanding
  bool ahead_off = false;               // the sets could not be allocated: the calls stay in order
  // device regions that hold secret-key material during the current call (sk coefficients, NTT(sk), key errors,
  // their MFMA-tiled / digitised copies): cleared on the call's stream before the workspace goes back to the pool
  // (the reference's SecretKey is Zeroize + ZeroizeOnDrop, src/keys/secret_key.rs:20-30).  `wiped` remembers what
  // the last call that had any cleared, for pvw_selftest_secret_residue.
  struct Span { void* p; size_t bytes; bool cleared; };
  std::vector<Span> secrets, wiped;
  // from this byte on the r-hat block holds the r-hat vectors of an encrypt (not key material), written since a key-bearing
  // call last marked that part: see ws_public.  A call that then marks the front of the block secret clears the front only.
  size_t rhat_public_from = SIZE_MAX;
};
// cleared: a kernel has cleared the region already (the wipe records it without a memset).  Marking a region again
// replaces its earlier mark.
static void ws_mark_secret(Workspace* w, void* p, size_t bytes, bool cleared = false) {
  if (!p || !bytes) return;
  if (p == (void*)w->rhat && w->rhat_public_from < bytes) w->rhat_public_from = bytes;
  for (Workspace::Span& sp : w->secrets)
    if (sp.p == p) { sp.bytes = bytes > sp.bytes ? bytes : sp.bytes; sp.cleared = cleared; return; }
  w->secrets.push_back(Workspace::Span{p, bytes, cleared});
}
// The current call is about to write data that is NOT key material into [p, p + bytes) of the workspace: the scratch block of a
// call that marks nothing there, the r-hat of an encrypt.  A pooled workspace goes from one kind of call to another, so the
// block may be what an earlier call declared secret and cleared; it is the new owner's now, and `wiped` (and the standing scan
// of the r-hat block) no longer answers for it -- pvw_selftest_secret_residue would count the new owner's data as a leftover
// key.  A region the current call itself holds as secret stays so.
static void ws_public(Workspace* w, void* p, size_t bytes) {
  if (!p || !bytes) return;
  const char *lo = (const char*)p, *hi = lo + bytes;
  for (const Workspace::Span& sp : w->secrets)
    if ((const char*)sp.p >= lo && (const char*)sp.p < hi) return;
  size_t kept = 0;
  for (const Workspace::Span& sp : w->wiped)
    if ((const char*)sp.p < lo || (const char*)sp.p >= hi) w->wiped[kept++] = sp;
  w->wiped.resize(kept);
  if (p == (void*)w->rhat) w->rhat_public_from = 0;
}
// enqueue the wipes on `s` (call after the last kernel that reads the regions has been enqueued on `s`); nothing
// marked: nothing enqueued, and the record of the last wipe stays
// Under stream capture the wipes are kernels, not memset nodes: a captured call has to clear its regions on every replay, in
// order (pvw_selftest_secret_residue after a replay found regions cleared by memset nodes not cleared).
static hipError_t ws_wipe_secrets(Workspace* w, hipStream_t s) {
  if (w->secrets.empty()) return hipSuccess;
  hipError_t rc = hipSuccess;
  const bool by_kernel = stream_capturing(s);
  for (const Workspace::Span& sp : w->secrets) {
    hipError_t e = hipSuccess;
    if (!sp.cleared) e = by_kernel && sp.bytes % 8 == 0 ? launch_wipe_words((u64*)sp.p, sp.bytes / 8, s) : hipMemsetAsync(sp.p, 0, sp.bytes, s);
    if (e != hipSuccess) rc = e;
  }
  w->wiped = w->secrets;
  w->secrets.clear();
  return rc;
}

struct pvw_ctx {
  u32 n, k, l, L;
  std::vector<u64> moduli, psi;
  float variance;
  u64 b1, b2;
  u32 num_cus = 256;               // of the context's device (set by ensure_device)
  u32 xm_bytes = 8;                // bytes per element in the MFMA-tiled copies xmA / xmB (set when they are built)
  int device;
  u32 party_lo, party_hi, c1_lo, c1_hi;
  BigInt Q, halfQ, delta, delta_pow;
  std::vector<BigInt> crt_qi;    // Q / q_i
  std::vector<u64> crt_inv;      // (Q/q_i)^-1 mod q_i
  std::vector<Mod> mods;
  std::vector<u64> tw, itw, linv, ghat, gpow;
  bool roots_locked = false;
  // fixed-width decode tables (host copies; pvw_decode.h)
  std::vector<u64> dec_words;      // all u64 tables back to back
  DecodeTables dec_host{};         // pointers into dec_words
  DecodeTables dec_dev{};          // pointers into d_dec
  void* d_dec = nullptr;

  // device state
  std::atomic<bool> dev_ready{false};
  void* d_tables = nullptr;
  DevTables dt{};
  u64* dA = nullptr;  // tiled A-hat rows [c1_lo, c1_hi)
  u64* dB = nullptr;  // tiled B-hat rows [party_lo, party_hi)
  // MFMA-tiled copies for the digit GEMM (built lazily by the first many-dealer encrypt, dropped
  // whenever A or B changes)
  u64* xmA = nullptr;
  u64* xmB = nullptr;
  bool xm_valid = false;
  // packed copies (pk_width = 40 / 48 / 56 / 61 bits per residue, by the widest modulus) for the single-dealer
  // mac_rows: built by pvw_prepare, or lazily by the first encrypt after the matrices changed, when the geometry
  // allows it and the memory is there (launch_pack); a section is rebuilt when ITS matrix changed
  u64* pkA = nullptr;
  u64* pkB = nullptr;
  u32* pk_flag = nullptr;   // device word: set by pack_kernel when a matrix word exceeds the stream width
  u32 pk_width = 0;         // 0: the geometry does not qualify (decided at context creation)
  bool pkA_valid = false, pkB_valid = false;
  bool pk_wide = false;     // the resident matrices hold unreduced words: no packed stream until they change
  u32 pk_nomem_calls = 0;   // encrypts since the copies last failed to fit (the allocation is retried now and then)
  bool crs_loaded = false;
  u32 num_keys = 0;
  hipStream_t stream = nullptr;

  std::mutex mu, init_mu;
  std::vector<Workspace*> pool;
  std::map<void*, Workspace*> async_ws;

  bool profiling = false;
  std::vector<ProfRec> prof;
  std::map<std::string, std::pair<double, uint64_t>> prof_acc;

  u32 rowsA() const { return c1_hi - c1_lo; }
  u32 rowsB() const { return party_hi - party_lo; }
  u32 R() const { return 128 / l; }
  size_t poly() const { return (size_t)L * l; }
  size_t tiled_words(u32 rows) const { return (size_t)((rows + R() - 1) / R()) * L * k * 128; }
};

struct ProfScope {
  pvw_ctx* c;
  hipStream_t s;
  ProfRec rec;
  bool on;
  ProfScope(pvw_ctx* c_, const char* name, hipStream_t s_) : c(c_), s(s_), on(c_->profiling) {
    if (on) {
      rec.name = name;
      hipEventCreate(&rec.a);
      hipEventCreate(&rec.b);
      hipEventRecord(rec.a, s);
    }
  }
  ~ProfScope() {
    if (on) {
      hipEventRecord(rec.b, s);
      std::lock_guard<std::mutex> g(c->mu);
      c->prof.push_back(rec);
    }
  }
};

static void build_tables(pvw_ctx* c) {
  const u32 L = c->L, l = c->l, bits = ilog2(l);
  c->tw.assign((size_t)L * l, 0);
  c->itw.assign((size_t)L * l, 0);
  c->linv.assign(L, 0);
  c->gpow.assign((size_t)L * l, 0);
  c->ghat.assign((size_t)L * l, 0);
  for (u32 i = 0; i < L; ++i) {
    const Mod& m = c->mods[i];
    u64 psi = c->psi[i], ipsi = powmod(psi, m.q - 2, m);
    for (u32 x = 0; x < l; ++x) {
      c->tw[(size_t)i * l + x] = powmod(psi, bitrev32(x, bits), m);
      c->itw[(size_t)i * l + x] = powmod(ipsi, bitrev32(x, bits), m);
    }
    c->linv[i] = powmod(l, m.q - 2, m);
    // gadget residues D^j mod q_i (parameters.rs:288-308) and their NTT
    u64 dm = c->delta.mod_small(m.q), p = 1;
    for (u32 j = 0; j < l; ++j) {
      c->gpow[(size_t)i * l + j] = p;
      p = mulmod(p, dm, m);
    }
    std::vector<u64> g(c->gpow.begin() + (size_t)i * l, c->gpow.begin() + (size_t)(i + 1) * l);
    host_ntt_forward(g.data(), l, &c->tw[(size_t)i * l], m);
    std::copy(g.begin(), g.end(), c->ghat.begin() + (size_t)i * l);
  }
}

static double correctness_bound(double n, double k, double l, double b1, double b2) {  // parameters.rs:510-544
  double first = b2 * std::sqrt(n * l) * (1.0 + std::sqrt(n));
  double second = 2.0 * b1 * k * l;
  double third = 14.0 * b1 * std::sqrt(n * k * l);
  return first + second + third;
}

// ---- decode tables (pvw_decode.h): big constants as W little-endian words ----
static void bn_words(const BigInt& v, size_t W, u64* out) {
  for (size_t i = 0; i < W; ++i) out[i] = i < v.mag.size() ? v.mag[i] : 0;
}
static void build_decode_tables(pvw_ctx* c) {
  const size_t L = c->L;
  const size_t W = (c->Q.bits() + 8 + 63) / 64;
  // layout (u64 words): Q | halfQ | qi[L][W] | inv[L] | invp[L] | pow64[L][W] | dmod[L] | dmodp[L] |
  //                     delta | dpow | half_dpow | dpow_n | td_n
  const size_t total = 2 * W + L * W + 2 * L + L * W + 2 * L + 5 * W + W * L + 3 * (W + 2) + 56 + 9 + 4 * L;
  c->dec_words.assign(total, 0);
  u64* p = c->dec_words.data();
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += n; return o; };
  const size_t oQ = take(W), oH = take(W), oQi = take(L * W), oInv = take(L), oInvp = take(L), oPow = take(L * W),
               oDm = take(L), oDmp = take(L), oDelta = take(W), oDpow = take(W), oHalfD = take(W), oDpn = take(W), oTdn = take(W),
               oPowT = take(W * L), oTd = take(W + 2), oMuTd = take(W + 2), oMuDp = take(W + 2), oGar = take(56), oSc = take(9), oDpm = take(4 * L);
  bn_words(c->Q, W, p + oQ);
  bn_words(c->halfQ, W, p + oH);
  for (size_t i = 0; i < L; ++i) {
    const Mod& m = c->mods[i];
    bn_words(c->crt_qi[i], W, p + oQi + i * W);
    p[oInv + i] = c->crt_inv[i];
    p[oInvp + i] = shoup_precompute(c->crt_inv[i], m.q);
    u64 b = powmod(2, 64, m), cur = 1;
    for (size_t j = 0; j < W; ++j) { p[oPow + i * W + j] = cur; cur = mulmod(cur, b, m); }
    u64 dm = c->delta.mod_small(m.q);
    p[oDm + i] = dm;
    p[oDmp + i] = shoup_precompute(dm, m.q);
  }
  for (size_t i = 0; i < L; ++i)
    for (size_t j = 0; j < W; ++j) p[oPowT + j * L + i] = p[oPow + i * W + j];
  {
    BigInt td = c->delta * BigInt(2), bw1 = BigInt(1).shl(64 * (W + 1));
    bn_words(td, W + 2, p + oTd);
    bn_words(bw1 / td, W + 2, p + oMuTd);
    bn_words(bw1 / c->delta_pow, W + 2, p + oMuDp);
  }
  bn_words(c->delta, W, p + oDelta);
  bn_words(c->delta_pow, W, p + oDpow);
  bn_words(c->delta_pow.shr(1), W, p + oHalfD);
  auto norm = [&](const BigInt& v, u64* dst, u32& nw, u32& sh) {
    nw = (u32)v.mag.size();
    sh = (u32)__builtin_clzll(v.mag.back());
    bn_words(v.shl(sh), W, dst);
  };
  DecodeTables t{};
  t.W = (u32)W; t.L = c->L; t.ell = c->l;
  norm(c->delta_pow, p + oDpn, t.dpow_nw, t.dpow_sh);
  norm(c->delta * BigInt(2), p + oTdn, t.td_nw, t.td_sh);
  // Garner constants of the short-cut lift (pvw_decode_wave.h).  A well-formed ciphertext's chain inputs are at most about
  // Delta times the decryption noise; the noise is below the bound of the correctness gate (parameters.rs:510-544).  Use as
  // many of the leading moduli as make half their product cover that with a few bits to spare: at least 2, at most 4, and
  // at least one limb must remain to confirm a candidate against.  (Whatever does not fit takes the full lift: the choice
  // only decides how often the short cut applies.)
  t.gar_n = 0;
  if (L >= 3) {
    const double bound = correctness_bound((double)c->n, (double)c->k, (double)c->l, (double)c->b1, (double)c->b2);
    const size_t need = c->delta.bits() + (size_t)std::ceil(std::log2(bound + 2.0)) + 4;
    const size_t most = std::min<size_t>(4, L - 1);
    u64* g = p + oGar;
    BigInt prod(1);
    size_t nl = 0;
    while (nl < most && (nl < 2 || prod.bits() < need + 1)) prod = prod * BigInt(c->moduli[nl++]);
    t.gar_n = (u32)nl;
    t.gar_close = 1;
    prod = BigInt(1);
    for (size_t j = 0; j <= nl; ++j) {
      bn_words(prod, 4, g + 32 + 4 * j);
      if (j == nl) break;
      for (size_t i = 0; i < j; ++i) {
        const u64 v = powmod(c->moduli[i] % c->moduli[j], c->moduli[j] - 2, c->mods[j]);
        g[4 * j + i] = v;
        g[16 + 4 * j + i] = shoup_precompute(v, c->moduli[j]);
        if (c->moduli[i] >= 2 * c->moduli[j]) t.gar_close = 0;
      }
      prod = prod * BigInt(c->moduli[j]);
    }
    bn_words(prod.shr(1), 4, g + 52);
  }
  // constants of the chain step on noise-sized operands: an operand below 2^191 on either side keeps a - b inside
  // (-Q/2, Q/2) once Q has 194 bits, so the integer difference IS the centred difference the reference takes mod Q
  {
    const BigInt td = c->delta * BigInt(2);
    t.sc_on = (t.gar_n != 0 && c->Q.bits() >= 194 && td.mag.size() <= 3) ? 1 : 0;
    if (t.sc_on) {
      u64* sc = p + oSc;
      const size_t sh = 192 - td.bits();
      const BigInt td3 = td.shl(sh);
      bn_words(td3, 3, sc);
      const BigInt recip = (BigInt(1).shl(128) - BigInt(1)) / BigInt(sc[2]) - BigInt(1).shl(64);
      bn_words(recip, 1, sc + 3);
      sc[4] = sh / 64;
      sc[5] = sh % 64;
      bn_words(c->delta, 3, sc + 6);
    }
  }
  // Delta^(l-1) mod q_i, its inverse
  {
    bool all_inv = true;
    for (size_t i = 0; i < L; ++i) {
      const u64 q = c->moduli[i], v = c->delta_pow.mod_small(q);
      p[oDpm + i] = v;
      p[oDpm + L + i] = shoup_precompute(v, q);
      const u64 inv = v ? powmod(v, q - 2, c->mods[i]) : 0;
      if (!v) all_inv = false;
      p[oDpm + 2 * L + i] = inv;
      p[oDpm + 3 * L + i] = shoup_precompute(inv, q);
    }
    // e Delta^(l-1) + g must stay inside (-Q/2, Q/2) for every |e| <= q_0/2 < 2^61, |g| <= Delta/2
    const bool room = BigInt::cmp(c->halfQ, c->delta_pow.shl(61) + c->delta) > 0;
    t.hs_on = (t.sc_on && all_inv && room && c->l >= 3 && c->moduli[0] < (1ULL << 62)) ? 1 : 0;
  }
  t.ck_mul = BigInt::cmp(c->Q, c->delta.shl(64)) > 0 ? 1 : 0;   // Delta (2^64 - 1) < Q
  auto bind = [&](DecodeTables& d, const u64* base, const Mod* mods) {
    d = t;
    d.mods = mods;
    d.Q = base + oQ; d.halfQ = base + oH; d.qi = base + oQi; d.inv = base + oInv; d.invp = base + oInvp;
    d.pow64 = base + oPow; d.dmod = base + oDm; d.dmodp = base + oDmp; d.delta = base + oDelta;
    d.dpow = base + oDpow; d.half_dpow = base + oHalfD; d.dpow_n = base + oDpn; d.td_n = base + oTdn;
    d.pow64T = base + oPowT; d.td = base + oTd; d.mu_td = base + oMuTd; d.mu_dp = base + oMuDp; d.gar = base + oGar; d.sc = base + oSc; d.dpm = base + oDpm;
  };
  bind(c->dec_host, p, c->mods.data());
  c->dec_dev = t;   // pointers bound at upload
}

static int32_t upload_tables(pvw_ctx* c) {
  const size_t L = c->L, l = c->l;
  const size_t bytes = L * sizeof(Mod) + 8 * L * l * 8 + 2 * L * 8;
  if (!c->d_tables) PVW_HIP(hipMalloc(&c->d_tables, bytes));
  char* p = (char*)c->d_tables;
  auto put = [&](const void* src, size_t n) -> const void* {
    const void* at = p;
    hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    p += n;
    return at;
  };
  c->dt.mods = (const Mod*)put(c->mods.data(), L * sizeof(Mod));
  c->dt.min_q_bits = 64;
  c->dt.max_q_bits = 0;
  for (u32 i = 0; i < L; ++i) {
    u32 bits = 0;
    for (u64 q = c->mods[i].q; q; q >>= 1) ++bits;
    if (bits < c->dt.min_q_bits) c->dt.min_q_bits = bits;
    if (bits > c->dt.max_q_bits) c->dt.max_q_bits = bits;
  }
  c->dt.tw = (const u64*)put(c->tw.data(), L * l * 8);
  c->dt.itw = (const u64*)put(c->itw.data(), L * l * 8);
  c->dt.ghat = (const u64*)put(c->ghat.data(), L * l * 8);
  c->dt.gpow = (const u64*)put(c->gpow.data(), L * l * 8);
  c->dt.linv = (const u64*)put(c->linv.data(), L * 8);
  // Shoup companions floor(x * 2^64 / q)
  auto shoup = [&](const std::vector<u64>& src, size_t per_limb) {
    std::vector<u64> out(src.size());
    for (size_t i = 0; i < src.size(); ++i) out[i] = shoup_precompute(src[i], c->moduli[i / per_limb]);
    return out;
  };
  std::vector<u64> twp = shoup(c->tw, l), itwp = shoup(c->itw, l), ghatp = shoup(c->ghat, l),
                   gpowp = shoup(c->gpow, l), linvp = shoup(c->linv, 1);
  c->dt.twp = (const u64*)put(twp.data(), L * l * 8);
  c->dt.itwp = (const u64*)put(itwp.data(), L * l * 8);
  c->dt.ghatp = (const u64*)put(ghatp.data(), L * l * 8);
  c->dt.gpowp = (const u64*)put(gpowp.data(), L * l * 8);
  c->dt.linvp = (const u64*)put(linvp.data(), L * 8);
  // decode tables
  if (!c->d_dec) PVW_HIP(hipMalloc(&c->d_dec, c->dec_words.size() * 8));
  PVW_HIP(hipMemcpy(c->d_dec, c->dec_words.data(), c->dec_words.size() * 8, hipMemcpyHostToDevice));
  {
    const u64* hb = c->dec_words.data();
    const u64* db = (const u64*)c->d_dec;
    DecodeTables d = c->dec_host;
    auto mv = [&](const u64* hp) { return db + (hp - hb); };
    d.mods = c->dt.mods;
    d.Q = mv(d.Q); d.halfQ = mv(d.halfQ); d.qi = mv(d.qi); d.inv = mv(d.inv); d.invp = mv(d.invp); d.pow64 = mv(d.pow64);
    d.dmod = mv(d.dmod); d.dmodp = mv(d.dmodp); d.delta = mv(d.delta); d.dpow = mv(d.dpow); d.half_dpow = mv(d.half_dpow);
    d.dpow_n = mv(d.dpow_n); d.td_n = mv(d.td_n);
    d.pow64T = mv(d.pow64T); d.td = mv(d.td); d.mu_td = mv(d.mu_td); d.mu_dp = mv(d.mu_dp); d.gar = mv(d.gar); d.sc = mv(d.sc); d.dpm = mv(d.dpm);
    c->dec_dev = d;
  }
  PVW_HIP(hipDeviceSynchronize());
  return PVW_OK;
}

static int32_t ensure_device(pvw_ctx* c) {
  if (c->dev_ready) {
    PVW_HIP(hipSetDevice(c->device));
    return PVW_OK;
  }
  std::lock_guard<std::mutex> init_guard(c->init_mu);   // concurrent first calls initialise once
  if (c->dev_ready) {
    PVW_HIP(hipSetDevice(c->device));
    return PVW_OK;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(PVW_ERR_INTERNAL, "no HIP device available: the PVW hot path has no CPU fallback");
  if (c->device < 0) {
    int cur = 0;
    PVW_HIP(hipGetDevice(&cur));
    c->device = cur;
  }
  if (c->device >= count) return fail(PVW_ERR_INTERNAL, "device ordinal out of range");
  PVW_HIP(hipSetDevice(c->device));
  hipDeviceProp_t prop;
  PVW_HIP(hipGetDeviceProperties(&prop, c->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(PVW_ERR_INTERNAL, std::string("kernels are built for gfx950 only, device is ") +
                                      prop.gcnArchName);
  c->num_cus = (u32)prop.multiProcessorCount;
  PVW_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  PVW_HIP(init_kernel_attributes());          // per device: dynamic-LDS limits of the decode kernels
  PVW_HIP(init_wire_attributes());            // ... and of the wire codec
  PVW_HIP(init_shamir_attributes());          // ... and of the wide Berlekamp-Massey kernel
  PVW_TRY(upload_tables(c));
  c->dev_ready = true;
  c->roots_locked = true;
  return PVW_OK;
}

// Zeroes a block that has just been allocated and STAYS in use (recycled device memory may hold an earlier owner's data).
// hipMemset returns to the host before the fill has run, and the legacy default stream it runs on is not ordered against the
// workspaces' non-blocking streams: with that stream busy (a framework's work, other threads' fills) the fill landed AFTER the
// first kernels had written the block -- a deal then encrypted zeros for shares (tests/test_gpu_shamir_wide_concurrent.py,
// `default-stream`).  So the fill is waited for, once per block.  (A fill in front of hipFree needs no wait: hipFree waits.)
static hipError_t zero_fresh(void* p, size_t bytes) {
  const hipError_t e = hipMemset(p, 0, bytes);
  return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}

static int32_t ws_alloc(pvw_ctx* c, Workspace* w) {
  const size_t k = c->k, P = c->poly();
  PVW_HIP(hipMalloc((void**)&w->rhat, 4 * k * P * 8));   // up to 4 r-hat / s-hat vectors (mac_rows_multi)
  w->rhat_bytes = 4 * k * P * 8;
  PVW_HIP(zero_fresh(w->rhat, w->rhat_bytes));
  if (c->l <= 16) PVW_HIP(hipMalloc((void**)&w->esmall, ((size_t)c->rowsA() + c->rowsB()) * c->l * 8 + 16));
  return PVW_OK;
}
static int32_t ws_host_buffers(pvw_ctx* c, Workspace* w) {
  const size_t P = c->poly();
  if (!w->scalars) PVW_HIP(hipMalloc((void**)&w->scalars, (size_t)c->n * 8 + 16));
  if (!w->c1) PVW_HIP(hipMalloc((void**)&w->c1, (size_t)c->rowsA() * P * 8 + 16));
  if (!w->c2) PVW_HIP(hipMalloc((void**)&w->c2, (size_t)c->rowsB() * P * 8 + 16));
  return PVW_OK;
}
static int32_t ws_scratch(Workspace* w, size_t bytes) {
  ws_public(w, w->scratch, w->scratch_bytes);              // whatever the call marks secret in it comes back through its own wipe
  if (w->scratch_bytes >= bytes) return PVW_OK;
  // callers grow the scratch before they enqueue anything that uses it; whatever an earlier call left there is
  // cleared before the block goes back to the allocator
  if (w->scratch) { hipMemset(w->scratch, 0, w->scratch_bytes); hipFree(w->scratch); }
  w->wiped.clear();
  w->scratch = nullptr;
  w->scratch_bytes = 0;
  PVW_HIP(hipMalloc(&w->scratch, bytes));
  w->scratch_bytes = bytes;
  return PVW_OK;
}
// Grows one of the workspace's own buffers (dpart, sumbuf) to `need` bytes: `s`, whose queued work may still read the old
// block, is drained first; clear: the old block may hold key material.  (ws_scratch waits for nothing and resets `wiped`.)
static int32_t ws_grow(u64** buf, size_t* have, size_t need, hipStream_t s, bool clear) {
  if (*have >= need) return PVW_OK;
  if (*buf) {
    PVW_HIP(hipStreamSynchronize(s));
    if (clear) hipMemset(*buf, 0, *have);
    hipFree(*buf);
    *buf = nullptr;
    *have = 0;
  }
  PVW_HIP(hipMalloc((void**)buf, need));
  *have = need;
  return PVW_OK;
}
// The staging budget of the host-buffer calls: the bytes one staged piece may take on the device, 1 GiB.  Every bound below
// is a multiple of it (tuning build: PVW_STAGE_BYTES, read per call, so that the tests take several pieces at small shapes).
static size_t stage_budget() {
  const long b = PVW_ENV_INT("PVW_STAGE_BYTES", 0);
  return b > 0 ? (size_t)b : (size_t)1 << 30;
}
// items (dealers' ciphertext words, rows) per staged piece of at most 1 GiB: at least one, at most `most`
static size_t chunk_1gib(size_t item_bytes, size_t most) {
  const size_t per = stage_budget() / item_bytes;
  return per == 0 ? 1 : (per < most ? per : most);
}
static void ws_free(Workspace* w) {
  if (!w) return;
  // r-hat / s-hat vectors and the staging block may hold key material of the last call
  if (w->rhat && w->rhat_bytes) hipMemset(w->rhat, 0, w->rhat_bytes);
  if (w->scratch) hipMemset(w->scratch, 0, w->scratch_bytes);
  hipFree(w->rhat);
  hipFree(w->esmall);
  hipFree(w->dpart);
  if (w->sumbuf) hipMemset(w->sumbuf, 0, w->sumbuf_bytes);   // may hold the noisy polynomial of the last aggregate decrypt
  hipFree(w->sumbuf);
  hipFree(w->scalars);
  hipFree(w->c1);
  hipFree(w->c2);
  hipFree(w->scratch);
  hipFree(w->vhat16);
  hipFree(w->yd);
  hipFree(w->sy);
  hipFree(w->gtmpA);
  hipFree(w->gtmpB);
  hipFree(w->gtmpK);
  if (w->shares) hipMemset(w->shares, 0, w->shares_bytes);   // the last deal's shares, if its wipe did not run
  hipFree(w->shares);
  hipFree(w->interp);
  hipFree(w->interp_wide);
  hipFree(w->packw);
  hipFree(w->packw_wide);
  hipFree(w->handover_wide);
  if (w->handover_io) hipMemset(w->handover_io, 0, w->handover_io_bytes);   // the last report, if its wipe did not run
  hipFree(w->handover_io);
  hipFree(w->handover);
  hipFree(w->handover_rows);
  if (w->correct) hipMemset(w->correct, 0, w->correct_bytes);   // M of the last call, if its wipe did not run
  hipFree(w->correct);
  if (w->correct_wide) hipMemset(w->correct_wide, 0, w->correct_wide_bytes);
  hipFree(w->correct_wide);
  for (hipEvent_t e : w->events) hipEventDestroy(e);
  if (w->ahead_block) hipMemset(w->ahead_block, 0, w->ahead_set_bytes * w->ahead.slots());   // r-hat and errors of the last encrypts
  hipFree(w->ahead_block);
  for (hipEvent_t e : w->ahead_done) hipEventDestroy(e);
  for (hipEvent_t e : w->ahead_guard) if (e) hipEventDestroy(e);
  if (w->ahead_mark) hipEventDestroy(w->ahead_mark);
  if (w->aux) hipStreamDestroy(w->aux);
  if (w->own_stream && w->stream) hipStreamDestroy(w->stream);
  delete w;
}
// synchronous host-buffer calls take a private workspace + stream from the pool
static int32_t ws_acquire(pvw_ctx* c, Workspace** out) {
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->pool.empty()) {
      *out = c->pool.back();
      c->pool.pop_back();
      return PVW_OK;
    }
  }
  Workspace* w = new Workspace();
  if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
    delete w;
    return fail(PVW_ERR_INTERNAL, "hipStreamCreate failed");
  }
  w->own_stream = true;
  int32_t rc = ws_alloc(c, w);
  if (rc != PVW_OK) { ws_free(w); return rc; }
  *out = w;
  return PVW_OK;
}
static void ws_release(pvw_ctx* c, Workspace* w) {
  std::lock_guard<std::mutex> g(c->mu);
  c->pool.push_back(w);
}
// asynchronous device-pointer calls keep one workspace per stream (stream order protects it)
static int32_t ws_for_stream(pvw_ctx* c, hipStream_t s, Workspace** out) {
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->async_ws.find((void*)s);
  if (it != c->async_ws.end()) { *out = it->second; return PVW_OK; }
  Workspace* w = new Workspace();
  w->stream = s;
  int32_t rc = ws_alloc(c, w);
  if (rc != PVW_OK) { ws_free(w); return rc; }
  c->async_ws[(void*)s] = w;
  *out = w;
  return PVW_OK;
}

// The scratch of one call: regions added in order, each rounded up to `align` bytes (256; the wire codec's 16).  `total`
// is what ws_scratch is asked for; at<T>(i) points into the block that take() bound.
// A call's results take their regions through Report::reserve and are addressed through Report::in.
struct Scratch {
  size_t align, total = 0;
  std::vector<size_t> off;
  char* base = nullptr;
  explicit Scratch(size_t a = 256) : align(a) {}
  size_t add(size_t bytes) {
    off.push_back(total);
    total += (bytes + align - 1) & ~(align - 1);
    return off.size() - 1;
  }
  int32_t take(Workspace* w) {
    PVW_TRY(ws_scratch(w, total));
    base = (char*)w->scratch;
    return PVW_OK;
  }
  template <class T = u64> T* at(size_t i) const { return (T*)(base + off[i]); }
  size_t bytes(size_t i) const { return (i + 1 < off.size() ? off[i + 1] : total) - off[i]; }   // rounded
  // regions i..j (one contiguous span) hold key material for the rest of the call
  void secret(Workspace* w, size_t i, size_t j) const { ws_mark_secret(w, base + off[i], off[j] + bytes(j) - off[i]); }
};

// What a decode reports for each result: out, and where asked for noise and status (the checked decode), the value
// mod `m` in out and the wide words [.][ww] (the plain decode).  One value stands for the caller's buffers (host or
// device) and, through in() / packed_at(), for the staging copy with the same fields.
struct Report {
  u64* out = nullptr;
  u64* noise = nullptr;
  u32* status = nullptr;
  u64* wide = nullptr;
  size_t ww = 0;
  Mod m{0, 0, 0};                                        // q = 0: no plain modulus
  template <class T> static T* from(T* p, size_t i) { return p ? p + i : nullptr; }
  // the same report starting at result i
  Report at(size_t i) const {
    Report r = *this;
    r.out = from(out, i), r.noise = from(noise, i), r.status = from(status, i), r.wide = from(wide, i * ww);
    return r;
  }
  // launch_decode's options: NULL when none is set (the checked decode then runs as it is)
  bool plain_on() const { return m.q || ww; }
  PlainArgs plain() const { return PlainArgs{m, (u32)ww, ww ? wide : nullptr}; }
  // Scratch regions for n results, always four and in this order: out | noise | status | wide; returns the first one's index
  static size_t reserve(Scratch& sc, size_t n, bool noise, bool status, size_t ww) {
    const size_t r = sc.add(n * 8);
    sc.add(noise ? n * 8 : 0), sc.add(status ? n * 4 : 0), sc.add(n * ww * 8);
    return r;
  }
  size_t reserve(Scratch& sc, size_t n) const { return reserve(sc, n, noise, status, ww); }
  // this report's fields in the regions reserved at r
  Report in(const Scratch& sc, size_t r) const {
    Report d = *this;
    d.out = sc.at(r), d.noise = noise ? sc.at(r + 1) : nullptr, d.status = status ? sc.at<u32>(r + 2) : nullptr;
    d.wide = ww ? sc.at(r + 3) : nullptr;
    return d;
  }
  // ... and back to back at `base`: out [n] | noise [n] | status [n] (4 bytes each, 8 reserved) | wide [n][ww]
  static size_t packed_bytes(size_t n, size_t ww) { return n * (24 + 8 * ww); }
  Report packed_at(u64* base, size_t n) const {
    Report d = *this;
    d.out = base, d.noise = noise ? base + n : nullptr, d.status = status ? (u32*)(base + 2 * n) : nullptr;
    d.wide = ww ? base + 3 * n : nullptr;
    return d;
  }
  // n results into dst, a report of the same fields (wide_first: the wide words ahead of out instead of behind status)
  int32_t copy_to(const Report& dst, size_t n, hipMemcpyKind kind, hipStream_t s, bool wide_first = false) const {
    if (ww && wide_first) PVW_HIP(hipMemcpyAsync(dst.wide, wide, n * ww * 8, kind, s));
    PVW_HIP(hipMemcpyAsync(dst.out, out, n * 8, kind, s));
    if (noise) PVW_HIP(hipMemcpyAsync(dst.noise, noise, n * 8, kind, s));
    if (status) PVW_HIP(hipMemcpyAsync(dst.status, status, n * 4, kind, s));
    if (ww && !wide_first) PVW_HIP(hipMemcpyAsync(dst.wide, wide, n * ww * 8, kind, s));
    return PVW_OK;
  }
  // a [rows][cols] block into dst, whose rows are D results apart
  int32_t copy_block_to(const Report& dst, size_t rows, size_t cols, size_t D, hipMemcpyKind kind, hipStream_t s) const {
    PVW_HIP(hipMemcpy2DAsync(dst.out, D * 8, out, cols * 8, cols * 8, rows, kind, s));
    if (noise) PVW_HIP(hipMemcpy2DAsync(dst.noise, D * 8, noise, cols * 8, cols * 8, rows, kind, s));
    if (status) PVW_HIP(hipMemcpy2DAsync(dst.status, D * 4, status, cols * 4, cols * 4, rows, kind, s));
    if (ww) PVW_HIP(hipMemcpy2DAsync(dst.wide, D * ww * 8, wide, cols * ww * 8, cols * ww * 8, rows, kind, s));
    return PVW_OK;
  }
};

// A device randomness state's handle (pvw_rnd_state_create, further down): it records the device and the stream of the context
// it was created for and never reads the context again.
struct pvw_rnd_state {
  int device;
  hipStream_t stream;   // the creating context's stream: NULL stream arguments and the clearing in pvw_rnd_state_free
  RndState* dev;
};
// after the argument checks of the call (the handle itself is not read before them)
static int32_t rnd_state_checks(const pvw_ctx* c, const pvw_rnd_state* st) {
  if (!st->dev) return fail(PVW_ERR_INVALID_PARAMETERS, "randomness state has been freed");
  if (c->rowsA() == 0 && c->rowsB() == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "the context holds no rows to encrypt");
  if (c->device >= 0 && st->device != c->device) return fail(PVW_ERR_INVALID_PARAMETERS, "the randomness state lives on another device");
  return PVW_OK;
}

// Where the dealers of an encrypt get their keys: dealer i of this value has host seed seeds[first + i] (32 bytes each), or
// call_seed(S, counter + first + i) of a device state, drawn when the kernels run.  An entry point builds it from its argument
// without reading the handle; checks() is the handle's first read.
struct DealerKeys {
  const uint8_t* seeds = nullptr;
  const pvw_rnd_state* st = nullptr;
  bool by_state = false;
  u64 first = 0;
  static DealerKeys host(const uint8_t* seeds) { return DealerKeys{seeds, nullptr, false, 0}; }
  static DealerKeys state(const void* handle) { return DealerKeys{nullptr, (const pvw_rnd_state*)handle, true, 0}; }
  bool missing() const { return by_state ? !st : !seeds; }
  int32_t checks(const pvw_ctx* c) const { return by_state ? rnd_state_checks(c, st) : (int32_t)PVW_OK; }
  // the state, for the counter advance that the last kernel of a call performs; NULL with host seeds
  RndState* state() const { return by_state ? st->dev : nullptr; }
  // the same source starting i dealers further on
  DealerKeys from(size_t i) const {
    DealerKeys k = *this;
    k.first += i;
    return k;
  }
  // ... for the staged piece of a host-buffer call that starts at dealer i: the pieces in front of it have advanced the
  // state's counter past their dealers, so only host seeds move on
  DealerKeys piece(size_t i) const { return by_state ? *this : from(i); }
  // the keys of dealers [0, count) into a kernel-side batch (PrologueBatch, GemmErrSource, ShamirBatch): count keys, or
  // the state and the offset of its first dealer
  template <class Batch>
  void fill(Batch& b, u32 count) const {
    if (by_state) {
      b.rnd = st->dev;
      b.rnd_off = first;
    } else {
      for (u32 x = 0; x < count; ++x) b.key[x] = make_key(seeds + (first + x) * 32);
    }
  }
};

// the helper stream and at least `events` events, for a call that runs on two streams
static int32_t ws_aux(Workspace* w, size_t events) {
  if (!w->aux) PVW_HIP(hipStreamCreateWithFlags(&w->aux, hipStreamNonBlocking));
  while (w->events.size() < events) {
    hipEvent_t e;
    PVW_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    w->events.push_back(e);
  }
  w->aux_used = true;
  return PVW_OK;
}

// Every host-buffer entry point runs its body here, on a pooled workspace and its stream.  However the body returns (early
// through PVW_HIP / PVW_TRY included), the helper stream is drained, the regions the body marked secret are cleared behind
// its last launch, the stream is drained, and only then does the workspace go back to the pool.  The first error wins.
template <class Body>
static int32_t host_call(pvw_ctx* c, Body&& body) {
  Workspace* w;
  PVW_TRY(ws_acquire(c, &w));
  int32_t rc = body(w);
  auto keep = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && rc == PVW_OK) rc = fail(PVW_ERR_INTERNAL, std::string(what) + " failed: " + hipGetErrorString(e));
  };
  if (w->aux_used) keep(hipStreamSynchronize(w->aux), "helper stream sync");
  w->aux_used = false;
  keep(ws_wipe_secrets(w, w->stream), "wipe");
  keep(hipStreamSynchronize(w->stream), "stream sync");
  ws_release(c, w);
  return rc;
}

// multi-dealer encrypt: the VALU below this many dealers, the matrix cores from it on
static bool multi_uses_gemm(size_t D) {
  const int gemm_min = (int)PVW_ENV_INT("PVW_GEMM_MIN_DEALERS", 3);   // tuning build: read per call (tests switch it); measured at config 3: 2 dealers 0.23 ms on the VALU vs 0.25 here, 4 dealers 0.43 vs 0.26, 6 dealers 0.67 vs 0.31
  return gemm_min > 0 && D >= (size_t)gemm_min;
}
// A device-pointer multi-dealer call made under stream capture may not allocate or wait: on the matrix cores it needs the
// MFMA copies and the stream's GEMM buffers that pvw_prepare(PVW_PREPARE_MFMA) builds.  Checked before the stream's workspace
// is looked up (a first call on a stream would allocate it) and before anything is enqueued, so the capture stays intact.
static int32_t multi_capture_check(pvw_ctx* c, hipStream_t s, size_t D) {
  if (!multi_uses_gemm(D) || !stream_capturing(s)) return PVW_OK;
  bool ready;
  {
    std::lock_guard<std::mutex> g(c->init_mu);
    ready = c->xm_valid;
  }
  {
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->async_ws.find((void*)s);
    const Workspace* w = it == c->async_ws.end() ? nullptr : it->second;
    ready = ready && w && w->vhat16 && w->yd && w->sy && (w->gtmpA || !c->rowsA()) && (w->gtmpB || !c->rowsB());
  }
  if (!ready)
    return fail(PVW_ERR_INVALID_PARAMETERS, "multi-dealer encrypt under stream capture: call pvw_prepare(PVW_PREPARE_MFMA) on "
                                            "this stream first (and again after the matrices change)");
  return PVW_OK;
}

// Under stream capture a deal may not allocate: the share scratch is built with the digit buffers by pvw_prepare(PVW_PREPARE_MFMA),
// whatever the dealer count (checked before the stream's workspace is looked up, like multi_capture_check)
static int32_t deal_capture_check(pvw_ctx* c, hipStream_t s, size_t D) {
  if (!stream_capturing(s)) return PVW_OK;
  bool ready;
  {
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->async_ws.find((void*)s);
    ready = it != c->async_ws.end() && it->second->shares;
  }
  if (!ready)
    return fail(PVW_ERR_INVALID_PARAMETERS, "multi-dealer encrypt under stream capture: call pvw_prepare(PVW_PREPARE_MFMA) on "
                                            "this stream first (and again after the matrices change)");
  return multi_capture_check(c, s, D);
}

// device-pointer calls: the caller's stream (NULL: the context's) and its workspace
static hipStream_t call_stream(const pvw_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }
static int32_t sum_prepare(pvw_ctx* c, Workspace* w, hipStream_t s);
static int32_t device_ws(pvw_ctx* c, void* stream, hipStream_t* s, Workspace** w) {
  *s = call_stream(c, stream);
  return ws_for_stream(c, *s, w);
}
// the end of a device-pointer call that marked key material: nothing of a failed call stays queued; the regions are
// cleared on the caller's stream behind the call's last launch (no wait on success)
static int32_t device_end(Workspace* w, hipStream_t s, int32_t rc) {
  if (rc != PVW_OK) {
    if (w->aux) (void)hipStreamSynchronize(w->aux);
    (void)hipStreamSynchronize(s);
  }
  if (ws_wipe_secrets(w, s) != hipSuccess && rc == PVW_OK) rc = fail(PVW_ERR_INTERNAL, "wipe failed");
  return rc;
}

// Every device-pointer entry point that marks key material, and every encrypt, runs its body here, host_call's counterpart:
// on the caller's stream and that stream's workspace, ended by device_end (which enqueues nothing for a call that marked
// nothing).  pre(s) runs BEFORE the workspace is looked up: the checks a call made under stream capture has to pass before
// anything is allocated (sum_capture_check, multi_capture_check), and an encrypt's first read of its randomness handle.
template <class Pre, class Body>
static int32_t device_call(pvw_ctx* c, void* stream, Pre&& pre, Body&& body) {
  PVW_TRY(ensure_device(c));
  const hipStream_t s = call_stream(c, stream);
  PVW_TRY(pre(s));
  Workspace* w;
  PVW_TRY(ws_for_stream(c, s, &w));
  return device_end(w, s, body(w, s));
}
template <class Body>
static int32_t device_call(pvw_ctx* c, void* stream, Body&& body) {
  return device_call(c, stream, [](hipStream_t) { return (int32_t)PVW_OK; }, body);
}

// ------------------------------------------------------------------------ parameters
static int32_t validate_params(const pvw_params_t* p) {
  if (!p) return fail(PVW_ERR_INVALID_PARAMETERS, "params is NULL");
  if (p->n == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "n must be > 0");                 // parameters.rs:132
  if (p->k == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "k must be > 0");                 // :135
  if (p->l < 8 || (p->l & (p->l - 1)) != 0)                                               // :140
    return fail(PVW_ERR_INVALID_PARAMETERS, "l must be power of 2 and >= 8 (fhe.rs Context requirement)");
  if (p->l > 64) return fail(PVW_ERR_INVALID_PARAMETERS, "l > 64 is not supported by the gfx950 kernels");
  if (p->num_moduli == 0 || !p->moduli) return fail(PVW_ERR_INVALID_PARAMETERS, "moduli not set");  // :129
  for (u32 i = 0; i < p->num_moduli; ++i) {
    u64 q = p->moduli[i];
    char buf[96];
    snprintf(buf, sizeof buf, "Context creation failed: modulus %#llx ", (unsigned long long)q);
    if (q >= (1ull << 62) || q < 3) return fail(PVW_ERR_INVALID_PARAMETERS, std::string(buf) + "must be in [3, 2^62)");
    if (!is_prime_u64(q)) return fail(PVW_ERR_INVALID_PARAMETERS, std::string(buf) + "is not prime");
    if ((q - 1) % (2 * (u64)p->l) != 0)
      return fail(PVW_ERR_INVALID_PARAMETERS, std::string(buf) + "is not 1 mod 2l (no NTT of size l)");
    for (u32 j = 0; j < i; ++j)
      if (p->moduli[j] == q) return fail(PVW_ERR_INVALID_PARAMETERS, std::string(buf) + "is repeated");
  }
  if (p->error_bound_1 == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "error_bound_1 must be positive");  // :172
  if (p->error_bound_2 == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "error_bound_2 must be positive");  // :177
  if (p->error_bound_1 >= (1ull << 62) || p->error_bound_2 >= (1ull << 62))
    return fail(PVW_ERR_INVALID_PARAMETERS, "error bounds must be below 2^62");
  return PVW_OK;
}

static void compute_q_delta(const u64* moduli, u32 L, u32 l, BigInt& Q, BigInt& delta, BigInt& dpow) {
  Q = BigInt(1);
  for (u32 i = 0; i < L; ++i) Q = Q * BigInt(moduli[i]);
  delta = Q.nth_root(l);            // parameters.rs:156
  dpow = delta.pow(l - 1);          // :159-163
}


extern "C" {

int32_t pvw_last_error(char* buf, size_t len) {
  if (!buf || len == 0) return PVW_ERR_INVALID_PARAMETERS;
  snprintf(buf, len, "%s", g_last_error.c_str());
  return PVW_OK;
}

int32_t pvw_device_available(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return 0;
  hipDeviceProp_t prop;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  return strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
}

int32_t pvw_ctx_create(const pvw_params_t* p, pvw_ctx** out) {
  if (!out) return fail(PVW_ERR_INVALID_PARAMETERS, "out is NULL");
  *out = nullptr;
  PVW_TRY(validate_params(p));
  pvw_ctx* c = new pvw_ctx();
  c->n = p->n; c->k = p->k; c->l = p->l; c->L = p->num_moduli;
  c->moduli.assign(p->moduli, p->moduli + p->num_moduli);
  c->variance = p->secret_variance;
  c->b1 = p->error_bound_1; c->b2 = p->error_bound_2;
  c->device = p->device;
  c->party_lo = p->party_lo; c->party_hi = p->party_hi;
  c->c1_lo = p->c1_lo; c->c1_hi = p->c1_hi;
  if (c->party_lo == 0 && c->party_hi == 0) c->party_hi = c->n;
  if (c->c1_lo == 0 && c->c1_hi == 0) c->c1_hi = c->k;
  if (c->party_lo > c->party_hi || c->party_hi > c->n || c->c1_lo > c->c1_hi || c->c1_hi > c->k) {
    delete c;
    return fail(PVW_ERR_INVALID_PARAMETERS, "party / c1 shard out of range");
  }
  compute_q_delta(c->moduli.data(), c->L, c->l, c->Q, c->delta, c->delta_pow);
  c->halfQ = c->Q.shr(1);
  for (u32 i = 0; i < c->L; ++i) {
    c->mods.push_back(make_mod(c->moduli[i]));
    c->psi.push_back(min_primitive_root(c->mods[i], 2 * c->l));
    BigInt qi = c->Q / BigInt(c->moduli[i]);
    c->crt_qi.push_back(qi);
    c->crt_inv.push_back(powmod(qi.mod_small(c->moduli[i]), c->moduli[i] - 2, c->mods[i]));
  }
  build_tables(c);
  build_decode_tables(c);
  {
    u32 maxbits = 0;
    for (u64 q : c->moduli) {
      u32 bits = 0;
      for (; q; q >>= 1) ++bits;
      if (bits > maxbits) maxbits = bits;
    }
    c->pk_width = packed_width(maxbits, c->k, c->l);
  }
  *out = c;
  return PVW_OK;
}

int32_t pvw_ctx_destroy(pvw_ctx* c) {
  if (!c) return PVW_OK;
  if (c->dev_ready) {
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (auto& r : c->prof) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (Workspace* w : c->pool) ws_free(w);
    for (auto& kv : c->async_ws) ws_free(kv.second);
    hipFree(c->dA);
    hipFree(c->dB);
    hipFree(c->xmA);
    hipFree(c->xmB);
    hipFree(c->pkA);
    hipFree(c->pkB);
    hipFree(c->pk_flag);
    hipFree(c->d_tables);
    hipFree(c->d_dec);
    if (c->stream) hipStreamDestroy(c->stream);
  }
  delete c;
  return PVW_OK;
}

int32_t pvw_ctx_get_roots(const pvw_ctx* c, uint64_t* psi_out) {
  if (!c || !psi_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  memcpy(psi_out, c->psi.data(), c->L * 8);
  return PVW_OK;
}

int32_t pvw_ctx_set_roots(pvw_ctx* c, const uint64_t* psi) {
  if (!c || !psi) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (c->roots_locked)
    return fail(PVW_ERR_CONTEXT, "roots must be set before any device operation");
  for (u32 i = 0; i < c->L; ++i)
    if (psi[i] >= c->moduli[i] || powmod(psi[i], c->l, c->mods[i]) != c->moduli[i] - 1)
      return fail(PVW_ERR_INVALID_PARAMETERS, "psi is not a primitive 2l-th root of unity");
  c->psi.assign(psi, psi + c->L);
  build_tables(c);
  return PVW_OK;
}

static int32_t export_big(const BigInt& v, uint64_t* words, size_t cap, size_t* nwords) {
  if (!nwords) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *nwords = v.mag.size();
  if (words) {
    if (cap < v.mag.size()) return fail(PVW_ERR_INSUFFICIENT_DATA, "word buffer too small");
    memcpy(words, v.mag.data(), v.mag.size() * 8);
  }
  return PVW_OK;
}
int32_t pvw_ctx_delta(const pvw_ctx* c, uint64_t* w, size_t cap, size_t* n) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  return export_big(c->delta, w, cap, n);
}
int32_t pvw_ctx_delta_power_l_minus_1(const pvw_ctx* c, uint64_t* w, size_t cap, size_t* n) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  return export_big(c->delta_pow, w, cap, n);
}
int32_t pvw_ctx_q_total(const pvw_ctx* c, uint64_t* w, size_t cap, size_t* n) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  return export_big(c->Q, w, cap, n);
}

int32_t pvw_ctx_gadget(const pvw_ctx* c, uint64_t* poly_out, uint32_t repr) {
  if (!c || !poly_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const std::vector<u64>& src = repr == PVW_REPR_NTT ? c->ghat : c->gpow;
  memcpy(poly_out, src.data(), src.size() * 8);
  return PVW_OK;
}

int32_t pvw_ctx_verify_correctness_condition(const pvw_ctx* c, int32_t* ok) {
  if (!c || !ok) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  double bound = correctness_bound((double)c->n, (double)c->k, (double)c->l, (double)c->b1, (double)c->b2);
  *ok = c->delta_pow.to_double() > bound ? 1 : 0;   // parameters.rs:547-550 (to_f64 saturates to +inf)
  return PVW_OK;
}

// total_bound of verify_correctness_condition (parameters.rs:516-543), the f64 sum floored and saturated to u64
int32_t pvw_ctx_noise_bound(const pvw_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const double b = std::floor(correctness_bound((double)c->n, (double)c->k, (double)c->l, (double)c->b1, (double)c->b2));
  *out = !(b >= 0.0) ? 0 : (b >= 18446744073709551616.0 ? ~(uint64_t)0 : (uint64_t)b);
  return PVW_OK;
}

int32_t pvw_suggest_error_bounds(uint32_t n, uint32_t k, uint32_t l, const uint64_t* moduli,
                                 uint32_t num_moduli, float variance, uint32_t* b1o, uint32_t* b2o) {
  if (!b1o || !b2o) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  pvw_params_t p{};
  p.n = n; p.k = k; p.l = l; p.moduli = moduli; p.num_moduli = num_moduli;
  p.secret_variance = variance; p.error_bound_1 = 1; p.error_bound_2 = 1; p.device = -1;   // parameters.rs:562-569
  PVW_TRY(validate_params(&p));
  BigInt Q, d, dp;
  compute_q_delta(moduli, num_moduli, l, Q, d, dp);
  const double dpf = dp.to_double();
  const double nf = n, kf = k, lf = l;
  const double c1 = 2.0 * kf * lf + 14.0 * std::sqrt(nf * kf * lf);      // :578-580
  const double c2 = std::sqrt(nf * lf) * (1.0 + std::sqrt(nf));          // :583-585
  static const uint32_t cand[] = {50, 100, 200, 500, 1000, 2000};
  for (uint32_t e1 : cand)
    for (uint32_t e2 : cand)
      if (dpf > (double)e1 * c1 + (double)e2 * c2) { *b1o = e1; *b2o = e2; return PVW_OK; }   // :588-598
  char buf[160];
  snprintf(buf, sizeof buf, "Cannot find suitable error bounds for variance %g with the correctness condition", variance);
  return fail(PVW_ERR_INVALID_PARAMETERS, buf);
}

int32_t pvw_ctx_resident_bytes(const pvw_ctx* c, uint64_t* crs, uint64_t* pk) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  if (crs) *crs = c->tiled_words(c->rowsA()) * 8;
  if (pk) *pk = c->tiled_words(c->rowsB()) * 8;
  return PVW_OK;
}

int32_t pvw_ctx_derived_bytes(const pvw_ctx* c, uint64_t* packed, uint64_t* mfma_tiled) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  if (packed) *packed = ((c->pkA ? packed_words(c->rowsA(), c->k, c->L, c->l, c->pk_width) : 0) +
                         (c->pkB ? packed_words(c->rowsB(), c->k, c->L, c->l, c->pk_width) : 0)) * 8;
  if (mfma_tiled) *mfma_tiled = ((c->xmA ? xm_words(c->rowsA(), c->k, c->L, c->l) : 0) + (c->xmB ? xm_words(c->rowsB(), c->k, c->L, c->l) : 0)) * 8;
  return PVW_OK;
}

int32_t pvw_ctx_packed_active(const pvw_ctx* c, uint32_t* width) {
  if (!c || !width) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const bool valid = c->pk_width && !c->pk_wide && (c->pkA_valid || c->rowsA() == 0) && (c->pkB_valid || c->rowsB() == 0);
  *width = valid ? c->pk_width : 0;
  return PVW_OK;
}

int32_t pvw_ctx_synchronize(pvw_ctx* c) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  PVW_TRY(ensure_device(c));
  PVW_HIP(hipDeviceSynchronize());
  return PVW_OK;
}

// ------------------------------------------------------------------------ profiling
static void prof_resolve(pvw_ctx* c) {
  hipDeviceSynchronize();
  std::lock_guard<std::mutex> g(c->mu);
  for (auto& r : c->prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      auto& acc = c->prof_acc[r.name];
      acc.first += ms;
      acc.second += 1;
    }
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  c->prof.clear();
}
int32_t pvw_ctx_set_profiling(pvw_ctx* c, int32_t on) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  c->profiling = on != 0;
  return PVW_OK;
}
int32_t pvw_ctx_kernel_time(pvw_ctx* c, const char* name, double* total_ms, uint64_t* launches) {
  if (!c || !name) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (c->dev_ready) { hipSetDevice(c->device); prof_resolve(c); }
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->prof_acc.find(name);
  if (total_ms) *total_ms = it == c->prof_acc.end() ? 0.0 : it->second.first;
  if (launches) *launches = it == c->prof_acc.end() ? 0 : it->second.second;
  return PVW_OK;
}
int32_t pvw_ctx_reset_profiling(pvw_ctx* c) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  if (c->dev_ready) { hipSetDevice(c->device); prof_resolve(c); }
  std::lock_guard<std::mutex> g(c->mu);
  c->prof_acc.clear();
  return PVW_OK;
}

// ------------------------------------------------------------------------ CRS / public key residency
static int32_t ensure_matrix(pvw_ctx* c, u64** M, u32 rows) {
  if (*M || rows == 0) return PVW_OK;
  const size_t bytes = c->tiled_words(rows) * 8;
  PVW_HIP(hipMalloc((void**)M, bytes));
  PVW_HIP(hipMemsetAsync(*M, 0, bytes, c->stream));   // padding rows must read as zero
  PVW_HIP(hipStreamSynchronize(c->stream));
  return PVW_OK;
}

// rows [lo, hi) (global numbering) of a matrix whose shard is [shard_lo, shard_hi); d_src holds
// [hi-lo][k][L][l].  Rows outside the shard are skipped.
static int32_t load_rows_device(pvw_ctx* c, u64* M, u32 shard_lo, u32 shard_hi, u32 lo, u32 hi,
                                const u64* d_src, uint32_t repr, hipStream_t s) {
  const u32 a = lo > shard_lo ? lo : shard_lo, b = hi < shard_hi ? hi : shard_hi;
  if (a >= b) return PVW_OK;
  const size_t rowwords = (size_t)c->k * c->poly();
  ProfScope ps(c, "tile", s);
  PVW_HIP(launch_tile(d_src + (size_t)(a - lo) * rowwords, M, b - a, a - shard_lo, c->k, c->L, c->l,
                      repr == PVW_REPR_POWER, c->dt, s));
  return PVW_OK;
}
// host source, staged through a bounded device buffer
static int32_t load_rows_host(pvw_ctx* c, u64* M, u32 shard_lo, u32 shard_hi, u32 lo, u32 hi,
                              const u64* src, uint32_t repr) {
  const u32 a = lo > shard_lo ? lo : shard_lo, b = hi < shard_hi ? hi : shard_hi;
  if (a >= b) return PVW_OK;
  const size_t rowwords = (size_t)c->k * c->poly();
  size_t chunk = ((size_t)256 << 20) / (rowwords * 8);
  if (chunk == 0) chunk = 1;
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, (chunk < (size_t)(b - a) ? chunk : (size_t)(b - a)) * rowwords * 8));
    for (u32 r0 = a; r0 < b; r0 += (u32)chunk) {
      const u32 cnt = (b - r0) < chunk ? (b - r0) : (u32)chunk;
      PVW_HIP(hipMemcpyAsync(w->scratch, src + (size_t)(r0 - lo) * rowwords, cnt * rowwords * 8, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(load_rows_device(c, M, shard_lo, shard_hi, r0, r0 + cnt, (const u64*)w->scratch, repr, w->stream));
    }
    return PVW_OK;
  });
}
// dealers per gemm_digits launch: PVW_GEMM_VB batches of 16 (they share one pass over the matrix through L2)
static u32 gemm_vb() {   // tuning build: PVW_GEMM_VB
  static const u32 v = [] {
    const long x = PVW_ENV_INT("PVW_GEMM_VB", 8);
    return (u32)(x < 1 ? 1 : (x > 8 ? 8 : x));
  }();
  return v;
}
// the shares of one pass of dealers of pvw_deal_shares* (DESIGN 8.9): the largest group encrypt_multi_enqueue forms, 128 dealers
enum { SHARE_PASS = 128 };
static int32_t ws_share_buffer(pvw_ctx* c, Workspace* w) {
  if (w->shares) return PVW_OK;
  const size_t bytes = (size_t)SHARE_PASS * c->n * 8;
  PVW_HIP(hipMalloc((void**)&w->shares, bytes));
  w->shares_bytes = bytes;
  PVW_HIP(zero_fresh(w->shares, bytes));
  return PVW_OK;
}
static int32_t ws_gemm_buffers(pvw_ctx* c, Workspace* w) {
  const u32 vb = gemm_vb();
  PVW_TRY(ws_share_buffer(c, w));
  if (!w->vhat16) PVW_HIP(hipMalloc((void**)&w->vhat16, (size_t)16 * vb * c->k * c->poly() * 8));
  if (!w->yd) PVW_HIP(hipMalloc((void**)&w->yd, yd_bytes(16 * vb, c->k, c->L, c->l)));
  if (!w->sy) PVW_HIP(hipMalloc((void**)&w->sy, sy_bytes(16 * vb, c->L, c->l)));
  if (!w->gtmpA && c->rowsA()) PVW_HIP(hipMalloc((void**)&w->gtmpA, (size_t)vb * gemm_tmp_words(c->rowsA(), c->L, c->l) * 8));
  if (!w->gtmpB && c->rowsB()) PVW_HIP(hipMalloc((void**)&w->gtmpB, (size_t)vb * gemm_tmp_words(c->rowsB(), c->L, c->l) * 8));
  return PVW_OK;
}
// MFMA-tiled copies of the resident A-hat / B-hat sections
static int32_t ensure_xm(pvw_ctx* c, hipStream_t s) {
  std::lock_guard<std::mutex> g(c->init_mu);
  if (c->xm_valid) return PVW_OK;
  const u32 rA = c->rowsA(), rB = c->rowsB();
  const size_t wa = xm_words(rA, c->k, c->L, c->l), wb = xm_words(rB, c->k, c->L, c->l);
  if (!c->xmA && wa) PVW_HIP(hipMalloc((void**)&c->xmA, wa * 8));
  if (!c->xmB && wb) PVW_HIP(hipMalloc((void**)&c->xmB, wb * 8));
  if (wa) PVW_HIP(hipMemsetAsync(c->xmA, 0, wa * 8, s));
  if (wb) PVW_HIP(hipMemsetAsync(c->xmB, 0, wb * 8, s));
  // every modulus below 2^56 and k a multiple of 64: the copy holds 7 bytes per element (gemm_ktiles), and multi-dealer
  // encrypt contracts over 7/8 of the terms.  Tuning build: PVW_GEMM_BYTES=8 keeps all 8.
  c->xm_bytes = gemm7_ok(c->dt.max_q_bits, c->k) && PVW_ENV_INT("PVW_GEMM_BYTES", 7) != 8 ? 7 : 8;
  ProfScope ps(c, "mftile", s);
  PVW_HIP(launch_mftile(c->dA, true, c->xmA, rA, c->k, c->L, c->l, s, c->xm_bytes, c->dt.mods));
  PVW_HIP(launch_mftile(c->dB, true, c->xmB, rB, c->k, c->L, c->l, s, c->xm_bytes, c->dt.mods));
  PVW_HIP(hipStreamSynchronize(s));
  c->xm_valid = true;
  return PVW_OK;
}

// packed copies of the resident A-hat / B-hat sections for mac_rows (pvw_mac.hip, mac_rows_packed*_kernel): needs
// l <= 16, k a multiple of 64 (256 at 61 bits), every modulus below 2^61, and room for a second copy of the matrices.
// Returns the stream width, or 0 when the plain tiled matrices are to be streamed instead.  may_build = false (a
// stream capture is in progress): only says what is valid already, touches nothing.
static u32 ensure_packed(pvw_ctx* c, hipStream_t s, bool may_build = true, size_t* bytes_taken = nullptr) {
  // tuning build: A/B runs against the unpacked stream, and an explicit schedule of the unpacked kernel is honoured
  if (PVW_ENV_INT("PVW_MAC_PACKED", 1) == 0 || (PVW_ENV_INT("PVW_MAC_VARIANT", 0) != 0 && PVW_ENV_INT("PVW_MAC_VARIANT", 0) != 44)) return 0;
  if (c->pk_width == 0) return 0;
  std::lock_guard<std::mutex> g(c->init_mu);
  const u32 rA = c->rowsA(), rB = c->rowsB();
  if (c->pk_wide) return 0;
  if ((c->pkA_valid || rA == 0) && (c->pkB_valid || rB == 0)) return c->pk_width;
  if (!may_build) return 0;
  const size_t wa = packed_words(rA, c->k, c->L, c->l, c->pk_width), wb = packed_words(rB, c->k, c->L, c->l, c->pk_width);
  const size_t need = (c->pkA || !wa ? 0 : wa * 8) + (c->pkB || !wb ? 0 : wb * 8);
  if (need) {
    // memory was short the last time: look again every 64th encrypt, not on every call
    if (c->pk_nomem_calls && (c->pk_nomem_calls++ & 63) != 0) return 0;
    size_t free_b = 0, total_b = 0;
    bool ok = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= need + ((size_t)4 << 30);   // leave room for the callers' own buffers
    if (ok && !c->pkA && wa) ok = hipMalloc((void**)&c->pkA, wa * 8) == hipSuccess;
    if (ok && !c->pkB && wb) ok = hipMalloc((void**)&c->pkB, wb * 8) == hipSuccess;
    if (!ok) {
      // nothing half-built stays behind, and a failed hipMalloc does not poison the next launch's hipGetLastError()
      if (!c->pkA_valid) { hipFree(c->pkA); c->pkA = nullptr; }
      if (!c->pkB_valid) { hipFree(c->pkB); c->pkB = nullptr; }
      (void)hipGetLastError();
      if (c->pk_nomem_calls == 0) c->pk_nomem_calls = 1;
      return 0;
    }
    c->pk_nomem_calls = 0;
    if (bytes_taken) *bytes_taken += need;
  }
  if (!c->pk_flag && hipMalloc((void**)&c->pk_flag, sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipMemsetAsync(c->pk_flag, 0, sizeof(u32), s) != hipSuccess) return 0;
  {
    ProfScope ps(c, "pack", s);
    if (!c->pkA_valid && launch_pack(c->dA, c->pkA, rA, c->k, c->L, c->l, c->pk_width, c->pk_flag, s) != hipSuccess) return 0;
    if (!c->pkB_valid && launch_pack(c->dB, c->pkB, rB, c->k, c->L, c->l, c->pk_width, c->pk_flag, s) != hipSuccess) return 0;
  }
  u32 wide = 1;
  if (hipMemcpyAsync(&wide, c->pk_flag, sizeof(u32), hipMemcpyDeviceToHost, s) != hipSuccess) return 0;
  if (hipStreamSynchronize(s) != hipSuccess) return 0;
  if (wide) {                                             // residues were loaded unreduced: stream the tiled matrices as they are
    c->pk_wide = true;
    return 0;
  }
  c->pkA_valid = c->pkB_valid = true;
  return c->pk_width;
}

// The derived copies and the calling stream's workspace, built NOW: after this, pvw_encrypt_device /
// pvw_encrypt_multi_device on `stream` neither allocate nor synchronise until a matrix changes again (GlobalPublicKey's
// mutators take &mut self, public_key.rs:214-263: a change and a use never overlap).
int32_t pvw_prepare(pvw_ctx* c, uint32_t flags, void* stream, uint64_t* bytes_out) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  if (flags & ~(uint32_t)(PVW_PREPARE_PACKED | PVW_PREPARE_MFMA | PVW_PREPARE_SUM)) return fail(PVW_ERR_INVALID_PARAMETERS, "unknown prepare flag");
  PVW_TRY(ensure_device(c));
  if (!c->crs_loaded && flags != PVW_PREPARE_SUM) return fail(PVW_ERR_CRS, "CRS not loaded");   // the sums read no matrix
  hipStream_t s;
  Workspace* w;
  PVW_TRY(device_ws(c, stream, &s, &w));
  size_t taken = 0;
  if (flags & PVW_PREPARE_SUM) PVW_TRY(sum_prepare(c, w, s));
  if (flags & PVW_PREPARE_PACKED) (void)ensure_packed(c, s, true, &taken);       // 0 = does not qualify / no room: pvw_ctx_packed_active tells
  if (flags & PVW_PREPARE_MFMA) {
    const bool had_a = c->xmA != nullptr, had_b = c->xmB != nullptr;
    PVW_TRY(ws_gemm_buffers(c, w));
    PVW_TRY(ensure_xm(c, s));
    if (!had_a && c->xmA) taken += xm_words(c->rowsA(), c->k, c->L, c->l) * 8;
    if (!had_b && c->xmB) taken += xm_words(c->rowsB(), c->k, c->L, c->l) * 8;
  }
  PVW_HIP(hipStreamSynchronize(s));
  if (bytes_out) *bytes_out = taken;
  return PVW_OK;
}

static int32_t check_repr(uint32_t repr) {
  if (repr != PVW_REPR_POWER && repr != PVW_REPR_NTT) return fail(PVW_ERR_INVALID_FORMAT, "unknown representation");
  return PVW_OK;
}

// matrix A (the CRS) or B (the public key) is about to change: its MFMA-tiled and packed copies are stale, and whether
// the matrices hold unreduced words is not known until they are packed again
static void matrix_changed(pvw_ctx* c, bool crs) {
  c->xm_valid = false;
  (crs ? c->pkA_valid : c->pkB_valid) = false;
  c->pk_wide = false;
}

int32_t pvw_load_crs(pvw_ctx* c, const uint64_t* a, uint32_t repr) {
  if (!c || !a) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(ensure_device(c));
  matrix_changed(c, true);
  PVW_TRY(ensure_matrix(c, &c->dA, c->rowsA()));
  PVW_TRY(load_rows_host(c, c->dA, c->c1_lo, c->c1_hi, 0, c->k, a, repr));
  c->crs_loaded = true;
  return PVW_OK;
}
int32_t pvw_load_crs_device(pvw_ctx* c, const uint64_t* d_a, uint32_t repr, void* stream) {
  if (!c || !d_a) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(ensure_device(c));
  matrix_changed(c, true);
  PVW_TRY(ensure_matrix(c, &c->dA, c->rowsA()));
  PVW_TRY(load_rows_device(c, c->dA, c->c1_lo, c->c1_hi, 0, c->k, d_a, repr, call_stream(c, stream)));
  c->crs_loaded = true;
  return PVW_OK;
}
int32_t pvw_crs_generate(pvw_ctx* c, const uint8_t seed[32]) {
  if (!c || !seed) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(ensure_device(c));
  matrix_changed(c, true);
  PVW_TRY(ensure_matrix(c, &c->dA, c->rowsA()));
  {
    ProfScope ps(c, "fill_uniform", c->stream);
    PVW_HIP(launch_fill_uniform_tiled(c->dA, make_key(seed), DOM_CRS, c->rowsA(), 0, c->c1_lo, c->k, c->L,
                                      c->l, c->dt, c->stream));
  }
  PVW_HIP(hipStreamSynchronize(c->stream));
  c->crs_loaded = true;
  return PVW_OK;
}
// PvwCrs::new_from_tag (crs.rs:74-90): seed = the 8 little-endian bytes of DefaultHasher(tag + "CRS") repeated
// four times.  std's DefaultHasher is SipHash-1-3 with a zero key; `str::hash` feeds the bytes followed by 0xFF.
static u64 siphash(const uint8_t* m, size_t len, u64 k0, u64 k1, int c_rounds, int d_rounds) {
  u64 v0 = k0 ^ 0x736f6d6570736575ULL, v1 = k1 ^ 0x646f72616e646f6dULL, v2 = k0 ^ 0x6c7967656e657261ULL,
      v3 = k1 ^ 0x7465646279746573ULL;
  auto rotl = [](u64 x, int b) { return (x << b) | (x >> (64 - b)); };
  auto round = [&]() {
    v0 += v1; v1 = rotl(v1, 13); v1 ^= v0; v0 = rotl(v0, 32);
    v2 += v3; v3 = rotl(v3, 16); v3 ^= v2;
    v0 += v3; v3 = rotl(v3, 21); v3 ^= v0;
    v2 += v1; v1 = rotl(v1, 17); v1 ^= v2; v2 = rotl(v2, 32);
  };
  size_t i = 0;
  for (; i + 8 <= len; i += 8) {
    u64 w = 0;
    for (int b = 0; b < 8; ++b) w |= (u64)m[i + b] << (8 * b);
    v3 ^= w;
    for (int r = 0; r < c_rounds; ++r) round();
    v0 ^= w;
  }
  u64 w = (u64)(len & 0xff) << 56;
  for (int b = 0; i + b < len; ++b) w |= (u64)m[i + b] << (8 * b);
  v3 ^= w;
  for (int r = 0; r < c_rounds; ++r) round();
  v0 ^= w;
  v2 ^= 0xff;
  for (int r = 0; r < d_rounds; ++r) round();
  return v0 ^ v1 ^ v2 ^ v3;
}
int32_t pvw_selftest_siphash(const uint8_t* msg, size_t len, uint64_t k0, uint64_t k1, int32_t c_rounds, int32_t d_rounds,
                             uint64_t* out) {
  if ((!msg && len) || !out || c_rounds < 1 || d_rounds < 1) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = siphash(msg, len, k0, k1, c_rounds, d_rounds);
  return PVW_OK;
}
int32_t pvw_crs_seed_from_tag(const char* tag, uint8_t seed_out[32]) {
  if (!tag || !seed_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  std::string m = std::string(tag) + "CRS";
  m.push_back((char)0xFF);                                   // the terminator `impl Hash for str` writes
  const u64 h = siphash((const uint8_t*)m.data(), m.size(), 0, 0, 1, 3);
  for (int i = 0; i < 32; ++i) seed_out[i] = (uint8_t)(h >> (8 * (i % 8)));
  return PVW_OK;
}

// SELF-TEST (host only): the constants behind the short cuts of the device decode (DecodeTables::gar / sc / dpm, built in
// build_decode_tables) against their defining identities, recomputed here with the host big integers.  info_out[0..3] =
// gar_n, gar_close, sc_on, hs_on -- which short cuts the parameter set reaches.
int32_t pvw_selftest_decode_tables(const pvw_ctx* c, uint32_t info_out[4]) {
  if (!c || !info_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const DecodeTables& t = c->dec_host;
  info_out[0] = t.gar_n; info_out[1] = t.gar_close; info_out[2] = t.sc_on; info_out[3] = t.hs_on;
  auto words = [](const u64* w, size_t n) { return BigInt::from_words(w, n); };
  if (t.gar_n) {
    if (t.gar_n < 2 || t.gar_n > 4 || t.gar_n >= c->L) return fail(PVW_ERR_INTERNAL, "decode tables: gar_n out of range");
    BigInt prod(1);
    bool close = true;
    for (u32 j = 0; j <= t.gar_n; ++j) {
      if (BigInt::cmp(words(t.gar + 32 + 4 * j, 4), prod) != 0) return fail(PVW_ERR_INTERNAL, "decode tables: partial product");
      if (j == t.gar_n) break;
      const u64 qj = c->moduli[j];
      for (u32 i = 0; i < j; ++i) {
        const u64 inv = t.gar[4 * j + i];
        if (inv >= qj || mulmod(inv, c->moduli[i] % qj, c->mods[j]) != 1) return fail(PVW_ERR_INTERNAL, "decode tables: mixed-radix inverse");
        if (t.gar[16 + 4 * j + i] != shoup_precompute(inv, qj)) return fail(PVW_ERR_INTERNAL, "decode tables: Shoup companion");
        if (c->moduli[i] >= 2 * qj) close = false;
      }
      prod = prod * BigInt(qj);
    }
    if (BigInt::cmp(words(t.gar + 52, 4), prod.shr(1)) != 0) return fail(PVW_ERR_INTERNAL, "decode tables: half product");
    if ((t.gar_close != 0) != close) return fail(PVW_ERR_INTERNAL, "decode tables: gar_close");
  }
  const BigInt td = c->delta * BigInt(2);
  if (t.sc_on) {
    if (!t.gar_n || c->Q.bits() < 194 || td.mag.size() > 3) return fail(PVW_ERR_INTERNAL, "decode tables: sc_on without its conditions");
    const size_t sh = 192 - td.bits();
    if (t.sc[4] != sh / 64 || t.sc[5] != sh % 64 || !(t.sc[2] >> 63)) return fail(PVW_ERR_INTERNAL, "decode tables: divisor shift");
    if (BigInt::cmp(words(t.sc, 3), td.shl(sh)) != 0) return fail(PVW_ERR_INTERNAL, "decode tables: normalised divisor");
    const BigInt recip = (BigInt(1).shl(128) - BigInt(1)) / BigInt(t.sc[2]) - BigInt(1).shl(64);
    if (BigInt::cmp(words(t.sc + 3, 1), recip) != 0) return fail(PVW_ERR_INTERNAL, "decode tables: reciprocal");
    if (BigInt::cmp(words(t.sc + 6, 3), c->delta) != 0) return fail(PVW_ERR_INTERNAL, "decode tables: Delta words");
  }
  bool all_inv = true;
  for (u32 i = 0; i < c->L; ++i) {
    const u64 q = c->moduli[i], v = c->delta_pow.mod_small(q);
    if (t.dpm[i] != v || t.dpm[c->L + i] != shoup_precompute(v, q)) return fail(PVW_ERR_INTERNAL, "decode tables: Delta^(l-1) residue");
    if (!v) { all_inv = false; continue; }
    const u64 inv = t.dpm[2 * c->L + i];
    if (mulmod(inv, v, c->mods[i]) != 1 || t.dpm[3 * c->L + i] != shoup_precompute(inv, q)) return fail(PVW_ERR_INTERNAL, "decode tables: Delta^(l-1) inverse");
  }
  if (t.hs_on) {
    const bool room = BigInt::cmp(c->halfQ, c->delta_pow.shl(61) + c->delta) > 0;
    if (!t.sc_on || !all_inv || !room || c->l < 3 || c->moduli[0] >= (1ULL << 62)) return fail(PVW_ERR_INTERNAL, "decode tables: hs_on without its conditions");
  }
  return PVW_OK;
}

int32_t pvw_build_is_tuning(void) { return PVW_TUNING; }

// SELF-TEST: 64-bit words that are not zero in the regions the last key-bearing call on each pooled workspace
// declared secret (and cleared), plus every workspace's r-hat / s-hat block.  0 after pvw_keygen / pvw_decrypt_*.
int32_t pvw_selftest_secret_residue(pvw_ctx* c, uint64_t* nonzero_words, uint64_t* scanned_words) {
  if (!c || !nonzero_words || !scanned_words) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *nonzero_words = *scanned_words = 0;
  if (!c->dev_ready) return PVW_OK;
  PVW_HIP(hipSetDevice(c->device));
  PVW_HIP(hipDeviceSynchronize());
  std::vector<Workspace*> all;
  {
    std::lock_guard<std::mutex> g(c->mu);
    all = c->pool;
    for (auto& kv : c->async_ws) all.push_back(kv.second);
  }
  std::vector<u64> host;
  for (Workspace* w : all) {
    std::vector<Workspace::Span> spans = w->wiped;
    if (w->rhat) spans.push_back(Workspace::Span{w->rhat, w->rhat_bytes < w->rhat_public_from ? w->rhat_bytes : w->rhat_public_from});
    for (const Workspace::Span& sp : spans) {
      const size_t step = (size_t)64 << 20;
      for (size_t off = 0; off < sp.bytes; off += step) {
        const size_t nb = (sp.bytes - off) < step ? (sp.bytes - off) : step;
        host.resize((nb + 7) / 8);
        host.back() = 0;
        PVW_HIP(hipMemcpy(host.data(), (const char*)sp.p + off, nb, hipMemcpyDeviceToHost));
        for (u64 v : host) *nonzero_words += v != 0;
        *scanned_words += host.size();
      }
    }
  }
  return PVW_OK;
}

static int32_t get_rows(pvw_ctx* c, const u64* M, u32 shard_lo, u32 shard_hi, u32 lo, u32 hi,
                        uint64_t* dst, uint32_t repr) {
  const u32 a = lo > shard_lo ? lo : shard_lo, b = hi < shard_hi ? hi : shard_hi;
  if (a >= b) return PVW_OK;
  if (!M) return fail(PVW_ERR_INVALID_PARAMETERS, "matrix not loaded");
  const size_t rowwords = (size_t)c->k * c->poly();
  size_t chunk = ((size_t)256 << 20) / (rowwords * 8);
  if (chunk == 0) chunk = 1;
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, (chunk < (size_t)(b - a) ? chunk : (size_t)(b - a)) * rowwords * 8));
    for (u32 r0 = a; r0 < b; r0 += (u32)chunk) {
      const u32 cnt = (b - r0) < chunk ? (b - r0) : (u32)chunk;
      PVW_HIP(launch_untile(M, (u64*)w->scratch, cnt, r0 - shard_lo, c->k, c->L, c->l, repr == PVW_REPR_POWER, c->dt, w->stream));
      PVW_HIP(hipMemcpyAsync(dst + (size_t)(r0 - lo) * rowwords, w->scratch, cnt * rowwords * 8, hipMemcpyDeviceToHost, w->stream));
    }
    return PVW_OK;
  });
}
int32_t pvw_get_crs(pvw_ctx* c, uint64_t* a_out, uint32_t repr) {
  if (!c || !a_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(ensure_device(c));
  return get_rows(c, c->dA, c->c1_lo, c->c1_hi, 0, c->k, a_out, repr);
}

static int32_t check_party_range(const pvw_ctx* c, u32 lo, u32 hi) {
  if (lo > hi) return fail(PVW_ERR_INVALID_PARAMETERS, "party_lo > party_hi");
  if (hi > c->n) {                                                                 // public_key.rs:216-222
    char buf[96];
    snprintf(buf, sizeof buf, "Party index %u exceeds maximum %u", hi - 1, c->n - 1);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  return PVW_OK;
}
int32_t pvw_load_pk(pvw_ctx* c, uint32_t lo, uint32_t hi, const uint64_t* b, uint32_t repr) {
  if (!c || !b) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(check_party_range(c, lo, hi));
  PVW_TRY(ensure_device(c));
  matrix_changed(c, false);
  PVW_TRY(ensure_matrix(c, &c->dB, c->rowsB()));
  PVW_TRY(load_rows_host(c, c->dB, c->party_lo, c->party_hi, lo, hi, b, repr));
  if (hi > c->num_keys) c->num_keys = hi;                                          // public_key.rs:245-247
  return PVW_OK;
}
int32_t pvw_load_pk_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const uint64_t* d_b, uint32_t repr, void* stream) {
  if (!c || !d_b) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(check_party_range(c, lo, hi));
  PVW_TRY(ensure_device(c));
  matrix_changed(c, false);
  PVW_TRY(ensure_matrix(c, &c->dB, c->rowsB()));
  PVW_TRY(load_rows_device(c, c->dB, c->party_lo, c->party_hi, lo, hi, d_b, repr, call_stream(c, stream)));
  if (hi > c->num_keys) c->num_keys = hi;
  return PVW_OK;
}
int32_t pvw_pk_fill_uniform(pvw_ctx* c, const uint8_t seed[32]) {
  if (!c || !seed) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(ensure_device(c));
  matrix_changed(c, false);
  PVW_TRY(ensure_matrix(c, &c->dB, c->rowsB()));
  {
    ProfScope ps(c, "fill_uniform", c->stream);
    PVW_HIP(launch_fill_uniform_tiled(c->dB, make_key(seed), DOM_PK, c->rowsB(), 0, c->party_lo, c->k, c->L,
                                      c->l, c->dt, c->stream));
  }
  PVW_HIP(hipStreamSynchronize(c->stream));
  c->num_keys = c->party_hi;
  return PVW_OK;
}
int32_t pvw_get_pk(pvw_ctx* c, uint32_t lo, uint32_t hi, uint64_t* b_out, uint32_t repr) {
  if (!c || !b_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(check_party_range(c, lo, hi));
  PVW_TRY(ensure_device(c));
  return get_rows(c, c->dB, c->party_lo, c->party_hi, lo, hi, b_out, repr);
}
int32_t pvw_num_public_keys(const pvw_ctx* c, uint32_t* out) {
  if (!c || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = c->num_keys;
  return PVW_OK;
}
int32_t pvw_is_full(const pvw_ctx* c, int32_t* out) {
  if (!c || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = c->num_keys >= c->party_hi ? 1 : 0;                                        // public_key.rs:349-351
  return PVW_OK;
}

// ------------------------------------------------------------------------ samplers
static int32_t cbd_job(float variance, SampleJob& j) {
  if (!(variance >= 0.5f && variance <= 16.0f))
    return fail(PVW_ERR_SAMPLING, "The variance should be between 0.5 and 16");          // uniform.rs:32-34
  j.kind = SAMPLE_CBD;
  j.cbd_half = std::fabs(variance - 0.5f) < 1.1920929e-07f ? 1 : 0;                       // :38
  j.cbd_v = (u32)variance;                                                                // :47
  if (!j.cbd_half && j.cbd_v < 1)
    return fail(PVW_ERR_SAMPLING, "non-integer variance below 1 is not supported (the reference's bit pool is empty there)");
  j.bound = 0;
  return PVW_OK;
}

// one sampling launch into scratch, copied to `out` (secret: the staged values are key material)
static int32_t sample_host(pvw_ctx* c, const char* name, size_t bytes, void* out, bool secret,
                           const std::function<hipError_t(i64*, hipStream_t)>& launch) {
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, bytes));
    if (secret) ws_mark_secret(w, w->scratch, bytes);
    {
      ProfScope ps(c, name, w->stream);
      PVW_HIP(launch((i64*)w->scratch, w->stream));
    }
    PVW_HIP(hipMemcpyAsync(out, w->scratch, bytes, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}

int32_t pvw_sample_cbd(pvw_ctx* c, const uint8_t seed[32], uint32_t domain, uint32_t index0, size_t count,
                       float variance, int64_t* out) {
  if (!c || !seed || (!out && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  SampleJob j{}, z{};
  PVW_TRY(cbd_job(variance, j));
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  j.domain = domain; j.index0 = index0; j.count = (u32)count; j.out_poly0 = 0;
  // SecretKey::random: the staged coefficients are key material
  return sample_host(c, "sample", count * c->l * 8, out, domain == PVW_DOM_SK,
                     [&](i64* d, hipStream_t s) { return launch_sample(d, make_key(seed), c->l, j, z, z, s); });
}

int32_t pvw_sample_uniform(pvw_ctx* c, const uint8_t seed[32], uint32_t domain, uint32_t index0, size_t count,
                           uint64_t bound, int64_t* out) {
  if (!c || !seed || (!out && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (bound >= (1ull << 62)) return fail(PVW_ERR_SAMPLING, "bound must be below 2^62");
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  SampleJob j{}, z{};
  j.kind = SAMPLE_UNIFORM; j.domain = domain; j.index0 = index0; j.count = (u32)count; j.bound = bound;
  return sample_host(c, "sample", count * c->l * 8, out, false,
                     [&](i64* d, hipStream_t s) { return launch_sample(d, make_key(seed), c->l, j, z, z, s); });
}

int32_t pvw_sample_gaussian(pvw_ctx* c, const uint8_t seed[32], uint32_t index0, size_t count, uint64_t bound,
                            int64_t* out) {
  if (!c || !seed || (!out && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (bound >= (1ull << 62)) return fail(PVW_ERR_SAMPLING, "bound must be below 2^62");
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  return sample_host(c, "gaussian", count * 8, out, false,
                     [&](i64* d, hipStream_t s) { return launch_gaussian(d, make_key(seed), index0, (u32)count, bound, s); });
}

int32_t pvw_sample_secret_keys(const pvw_ctx* cc, const uint8_t seed[32], uint32_t party_lo, uint32_t count,
                               int64_t* sk_out) {
  pvw_ctx* c = const_cast<pvw_ctx*>(cc);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL context");
  // party p, polynomial j uses stream index p*k + j
  return pvw_sample_cbd(c, seed, PVW_DOM_SK, party_lo * c->k, (size_t)count * c->k, c->variance, sk_out);
}
// a drawn key's stream index p * k + j is 32 bits wide
static int32_t check_sk_index(const pvw_ctx* c, uint64_t party_end) {
  if (party_end * c->k >= ((uint64_t)1 << 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "party_hi * k must be below 2^32 for seeded secret keys");
  return PVW_OK;
}
// the same words straight into the caller's device buffer on the caller's stream: one launch, no staging, no download, no
// synchronisation.  The buffer is the caller's to clear.
int32_t pvw_sample_secret_keys_device(pvw_ctx* c, const uint8_t seed[32], uint32_t party_lo, uint32_t count, int64_t* d_sk_out,
                                      void* stream) {
  if (!c || !seed || (!d_sk_out && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  SampleJob j{}, z{};
  PVW_TRY(cbd_job(c->variance, j));
  PVW_TRY(check_sk_index(c, (uint64_t)party_lo + count));
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  j.domain = DOM_SK; j.index0 = party_lo * c->k; j.count = count * c->k; j.out_poly0 = 0;
  hipStream_t s = call_stream(c, stream);
  ProfScope ps(c, "sample", s);
  PVW_HIP(launch_sample(d_sk_out, make_key(seed), c->l, j, z, z, s));
  return PVW_OK;
}

// ------------------------------------------------------------------------ ring primitives on host buffers
static int32_t ntt_host(pvw_ctx* c, uint64_t* polys, size_t count, bool inverse) {
  if (!c || (!polys && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const size_t bytes = count * c->poly() * 8;
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, bytes));
    PVW_HIP(hipMemcpyAsync(w->scratch, polys, bytes, hipMemcpyHostToDevice, w->stream));
    {
      ProfScope ps(c, inverse ? "intt" : "ntt", w->stream);
      PVW_HIP(launch_ntt((u64*)w->scratch, count, inverse, c->dt, c->L, c->l, w->stream));
    }
    PVW_HIP(hipMemcpyAsync(polys, w->scratch, bytes, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}
int32_t pvw_ntt_forward(pvw_ctx* c, uint64_t* polys, size_t count) { return ntt_host(c, polys, count, false); }
int32_t pvw_ntt_inverse(pvw_ctx* c, uint64_t* polys, size_t count) { return ntt_host(c, polys, count, true); }

static int32_t small_to_poly_impl(pvw_ctx* c, const int64_t* coeffs, const uint64_t* scalar, size_t count,
                                  uint64_t* polys, uint32_t repr) {
  PVW_TRY(check_repr(repr));
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  Scratch sc;
  const size_t r_in = sc.add(count * c->l * 8), r_out = sc.add(count * c->poly() * 8), r_sc = sc.add(scalar ? count * 8 : 0);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_HIP(hipMemcpyAsync(sc.at<i64>(r_in), coeffs, count * c->l * 8, hipMemcpyHostToDevice, w->stream));
    if (scalar) PVW_HIP(hipMemcpyAsync(sc.at(r_sc), scalar, count * 8, hipMemcpyHostToDevice, w->stream));
    {
      ProfScope ps(c, "prep", w->stream);
      PVW_HIP(launch_prep(sc.at<i64>(r_in), scalar ? sc.at(r_sc) : nullptr, sc.at(r_out), c->poly(), c->l, (u32)count,
                          repr == PVW_REPR_NTT, c->dt, c->L, c->l, w->stream));
    }
    PVW_HIP(hipMemcpyAsync(polys, sc.at(r_out), count * c->poly() * 8, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}
int32_t pvw_small_to_poly(pvw_ctx* c, const int64_t* coeffs, size_t count, uint64_t* polys, uint32_t repr) {
  if (!c || ((!coeffs || !polys) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  return small_to_poly_impl(c, coeffs, nullptr, count, polys, repr);
}
int32_t pvw_encode_scalar(const pvw_ctx* cc, int64_t scalar, uint64_t* poly_out, uint32_t repr) {
  pvw_ctx* c = const_cast<pvw_ctx*>(cc);
  if (!c || !poly_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  std::vector<int64_t> zero(c->l, 0);
  uint64_t s = (uint64_t)scalar;
  return small_to_poly_impl(c, zero.data(), &s, 1, poly_out, repr);
}

// the device's address for [p, p + bytes) if p is host memory the GPU can write (hipHostMalloc / hipHostRegister), else NULL
static void* device_alias(void* p, size_t bytes) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // pageable memory: not an error
  if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
  hipPointerAttribute_t last{};
  if (hipPointerGetAttributes(&last, (char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (last.type != hipMemoryTypeHost || (char*)last.devicePointer - (char*)at.devicePointer != (ptrdiff_t)(bytes - 1)) return nullptr;
  return at.devicePointer;
}

// host memory the device can read and write directly (pinned, mapped): output buffers placed here receive pvw_encrypt's
// ciphertexts without a copy
int32_t pvw_host_alloc(size_t bytes, void** out) {
  if (!out || bytes == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(PVW_ERR_INTERNAL, "no HIP device available");
  PVW_HIP(hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable));
  return PVW_OK;
}
int32_t pvw_host_free(void* p) {
  if (p) PVW_HIP(hipHostFree(p));
  return PVW_OK;
}

// ------------------------------------------------------------------------ encrypt
// explicit randomness of one encrypt: r [k][l], e1 [k][l], e2 [n][l] as GLOBAL arrays; all NULL: drawn from the dealer's key
struct ExplicitRnd {
  const i64 *r = nullptr, *e1 = nullptr, *e2 = nullptr;
  static ExplicitRnd of(const pvw_randomness_t* rnd) {
    return rnd && rnd->mode == PVW_RND_EXPLICIT ? ExplicitRnd{rnd->r, rnd->e1, rnd->e2} : ExplicitRnd{};
  }
};
// a seed form's key source: the seed field of its pvw_randomness_t (NULL: encrypt_checks refuses the call)
static DealerKeys seed_of(const pvw_randomness_t* rnd) { return DealerKeys::host(rnd ? rnd->seed : nullptr); }

// rnd: the seed forms' argument; the _rs forms (keys.by_state) have none
static int32_t encrypt_checks(pvw_ctx* c, size_t num_scalars, const pvw_randomness_t* rnd, const DealerKeys& keys, uint32_t out_repr) {
  PVW_TRY(check_repr(out_repr));
  if (!keys.by_state && !rnd) return fail(PVW_ERR_INVALID_PARAMETERS, "randomness is NULL");
  if (num_scalars != c->n) {                                                        // encryption.rs:109-115
    char buf[96];
    snprintf(buf, sizeof buf, "Must provide exactly n=%u scalars, got %zu", c->n, num_scalars);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (c->num_keys < c->party_hi)                                                    // :117-121
    return fail(PVW_ERR_INVALID_PARAMETERS, "Global public key is not complete (missing party keys)");
  if (!c->crs_loaded) return fail(PVW_ERR_CRS, "CRS not loaded");
  int32_t ok = 0;
  pvw_ctx_verify_correctness_condition(c, &ok);
  if (!ok)                                                                          // :124-128
    return fail(PVW_ERR_INVALID_PARAMETERS, "Parameters do not satisfy correctness condition - decryption may fail");
  if (keys.by_state) return PVW_OK;
  if (rnd->mode == PVW_RND_EXPLICIT) {
    if (!rnd->r || (!rnd->e1 && c->rowsA()) || (!rnd->e2 && c->rowsB()))
      return fail(PVW_ERR_INVALID_PARAMETERS, "explicit randomness pointers are NULL");
  } else if (rnd->mode != PVW_RND_SEED) {
    return fail(PVW_ERR_INVALID_PARAMETERS, "unknown randomness mode");
  }
  return PVW_OK;
}

// the three polynomial families of one encrypt (encryption.rs:135-154 r, :161-167 e1, :195-196
// encode + e2) as prologue jobs [3*slot, 3*slot+3) seeded by key `slot` of the batch, which the caller fills (DealerKeys::fill):
// r -> r-hat [L][k][l]; NTT(e1) -> c1 rows; NTT(e2) + scalar*g-hat -> c2 rows (the MAC adds onto them)
static int32_t fill_encrypt_jobs(pvw_ctx* c, PrologueBatch& pb, u32 slot, const ExplicitRnd& ex,
                                 const u64* d_scalars, u64* rhat, u64* d_c1, u64* d_c2) {
  const u32 k = c->k, l = c->l;
  const size_t P = c->poly();
  PrologueJob& jr = pb.job[3 * slot];
  PrologueJob& j1 = pb.job[3 * slot + 1];
  PrologueJob& j2 = pb.job[3 * slot + 2];
  jr = PrologueJob{}; j1 = PrologueJob{}; j2 = PrologueJob{};
  PVW_TRY(cbd_job(c->variance, jr.sj));
  jr.sj.domain = DOM_R; jr.sj.index0 = 0; jr.sj.count = k;
  j1.sj.kind = SAMPLE_UNIFORM; j1.sj.domain = DOM_E1; j1.sj.index0 = c->c1_lo; j1.sj.count = c->rowsA(); j1.sj.bound = c->b1;
  j2.sj.kind = SAMPLE_UNIFORM; j2.sj.domain = DOM_E2; j2.sj.index0 = c->party_lo; j2.sj.count = c->rowsB(); j2.sj.bound = c->b2;
  if (ex.r) {
    jr.explicit_coeffs = ex.r;
    j1.explicit_coeffs = ex.e1 + (size_t)c->c1_lo * l;
    j2.explicit_coeffs = ex.e2 + (size_t)c->party_lo * l;
  }
  jr.out = rhat; jr.stride_poly = l; jr.stride_limb = (size_t)k * l;
  j1.out = d_c1; j1.stride_poly = P; j1.stride_limb = l;
  j2.out = d_c2; j2.stride_poly = P; j2.stride_limb = l; j2.scalars = d_scalars + c->party_lo;
  jr.key_idx = j1.key_idx = j2.key_idx = slot;
  return PVW_OK;
}

// ---- the ahead path of a seed-mode encrypt ("The prologue and the step") ----
// How long the calling thread polls for the prologue on the side stream before it falls back to a wait packet in front of the
// MAC.  The poll ends when the prologue has run, which in steady state is when the MAC the side stream had to wait for has
// finished: at most one MAC of the flagship shape (0.18 ms) plus the prologue.
static constexpr long AHEAD_POLL_US = 1000;
// sets per bank of the ring (2R sets, one guard record on the caller's stream per R calls).  Measured at config 3 (profiles/
// r09_prologue_ahead_ab.txt, the shipped form): R = 1 steps 182.4 / 186.4 us, R = 4 184.3 / 187.1-187.7, R = 8 183.9 / 187.5-188.1
// (by MAC regime): fewer guard records buy nothing, and R = 1 keeps the calling thread at most two MACs ahead of the GPU.
// Tuning build: PVW_AHEAD_R, read when a stream's ring is first set up.
static constexpr unsigned AHEAD_R = 1;

// the caller's stream has something outstanding (asked only of a stream that is not capturing)
static bool stream_busy(hipStream_t s) {
  const hipError_t e = hipStreamQuery(s);
  (void)hipGetLastError();
  return e == hipErrorNotReady;
}
// The caller's stream has work outstanding, and enough of it to hide the wait: the MAC of the latest encrypt of this kind on
// the stream has not finished.  (stream_busy alone says too little: behind an event record or a small copy the stream is
// "not ready" for a few us, and a call that is alone there lost 15 us to the ahead path -- 207 against 192 us at config 3.)
static bool ahead_busy(const Workspace* w) {
  if (!w->ahead_last) return false;
  const hipError_t e = hipEventQuery(w->ahead_last);
  (void)hipGetLastError();
  return e == hipErrorNotReady;
}
// the workspace's ring, side stream and events, made by the first call that wants them; false: the call stays in order
static bool ahead_sets(pvw_ctx* c, Workspace* w) {
  if (w->ahead_off) return false;
  if (w->ahead_block) return true;
  w->ahead_off = true;                                   // until everything below has succeeded
  AheadRing ring;
  ring.reset((unsigned)PVW_ENV_INT("PVW_AHEAD_R", AHEAD_R));
  const size_t rhat_bytes = ((size_t)c->k * c->poly() * 8 + 255) & ~(size_t)255;
  const size_t set_bytes = rhat_bytes + ((((size_t)c->rowsA() + c->rowsB()) * c->l * 8 + 16 + 255) & ~(size_t)255);
  if (ws_aux(w, 0) != PVW_OK) { (void)hipGetLastError(); return false; }
  while (w->ahead_done.size() < ring.slots()) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
    w->ahead_done.push_back(e);
  }
  // The guards and the mark order no data: they say that a MAC has finished reading (the side stream may overwrite a set, the
  // host may go ahead), so they are recorded without a system-scope fence -- what the caller enqueues behind them fences for
  // itself.  Tuning build: PVW_AHEAD_FENCE=1 records them with the fence.
  const unsigned flags = hipEventDisableTiming | (PVW_ENV_INT("PVW_AHEAD_FENCE", 0) != 0 ? 0u : (unsigned)hipEventDisableSystemFence);
  for (hipEvent_t* e : {&w->ahead_guard[0], &w->ahead_guard[1], &w->ahead_mark})
    if (!*e && hipEventCreateWithFlags(e, flags) != hipSuccess) { *e = nullptr; (void)hipGetLastError(); return false; }
  void* block = nullptr;
  if (hipMalloc(&block, set_bytes * ring.slots()) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (zero_fresh(block, set_bytes * ring.slots()) != hipSuccess) { (void)hipGetLastError(); hipFree(block); return false; }
  w->ahead = ring;
  w->ahead_block = (char*)block;
  w->ahead_set_bytes = set_bytes;
  w->ahead_rhat_bytes = rhat_bytes;
  w->ahead_off = false;
  return true;
}
// polls until `ev` has completed; false: the bound ran out (or the query failed), the caller orders the streams by a wait.
// The calling thread SPINS here (no sleep: a wake-up costs more than the few us the MAC launch may be late by); in back-to-back
// use that is about one MAC per call, which also paces the caller: it runs at most two MACs ahead of the GPU.
static bool ahead_host_wait(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    if (e != hipErrorNotReady) return false;
    if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() >= AHEAD_POLL_US) return false;
  }
}

// all pointers are device pointers; explicit r/e1/e2 are GLOBAL arrays ([k][l], [k][l], [n][l])
// out_c1 / out_c2 != NULL: the MAC stores its results there (device-visible HOST memory of a caller whose buffers are
// pinned) while the addends stay in d_c1 / d_c2; NTT-domain output only
// keys: dealer 0's seed, or a device state: the prologue derives the key from it when it runs, and the MAC advances its
// counter by one
static int32_t encrypt_enqueue(pvw_ctx* c, Workspace* w, const u64* d_scalars, const DealerKeys& keys, const ExplicitRnd& ex,
                               u64* d_c1, u64* d_c2, uint32_t out_repr, hipStream_t s, u64* out_c1 = nullptr, u64* out_c2 = nullptr) {
  const u32 k = c->k, l = c->l, L = c->L, rA = c->rowsA(), rB = c->rowsB();
  if (!out_c1) out_c1 = d_c1;
  if (!out_c2) out_c2 = d_c2;
  if (out_repr == PVW_REPR_POWER && (out_c1 != d_c1 || out_c2 != d_c2)) return fail(PVW_ERR_INTERNAL, "direct output is NTT-domain only");
  // first call after a matrix change (and no pvw_prepare since): builds the packed copies -- allocates and synchronises
  const bool capturing = stream_capturing(s);
  const u32 width = ensure_packed(c, s, !capturing);
  // l <= 16: the addends travel in COMPACT form -- the prologue transforms r only and leaves the sampled e1 / e2 coefficients as
  // they are (8 l bytes per row instead of 8 L l written and read back); the MAC workgroups transform their own rows' e and add
  // m g-hat (MacSection::e_small, mac_small_make).  Explicit randomness: the caller's e1 / e2 arrays ARE the compact form.
  // (Round 3 also measured five forms of making r-hat and / or the addends inside the MAC launch instead of in a launch in front
  // of it: none was faster -- profiles/r03_front_ab.txt.)  Tuning build: PVW_MAC_COMPACT=0 the round-2 form (full addends).
  const bool compact = l <= 16 && w->esmall && PVW_ENV_INT("PVW_MAC_COMPACT", 1) != 0;
  // AHEAD: a seed-mode prologue with compact addends reads nothing but the seed, so only stream order would make it wait for
  // the work in front of it.  While the previous such encrypt's MAC is still outstanding on the caller's stream it runs on the
  // side stream instead, into the next set of the workspace's ring, and the calling thread waits for it (under the work already
  // queued) before it enqueues the MAC: the MAC then follows the one in front of it on `s` with no prologue and no wait packet
  // between them.  A stream with nothing of that size outstanding is a single call that wants its latency (in order: nobody
  // blocks); capture takes no host wait; the _rs prologue reads the counter the previous MAC advances; explicit randomness is
  // the caller's data; a host-buffer call's pooled stream is idle at every call.  Tuning build: PVW_PROLOGUE_AHEAD=0 keeps every
  // call in order.
  const bool can_ahead = compact && !ex.r && !keys.by_state && !capturing && !w->own_stream &&
                         PVW_ENV_INT("PVW_PROLOGUE_AHEAD", 1) != 0 && ahead_sets(c, w);
  const bool ahead = can_ahead && ahead_busy(w);
  // a call that stays in order leaves a mark behind its MAC for the next one only where the stream has something outstanding (a
  // burst is starting): behind a call that is alone on an idle stream the record would be 3-5 us in front of whatever follows
  const bool mark = can_ahead && (ahead || stream_busy(s));
  AheadRing::Step at{};
  u64* rhat = w->rhat;
  i64* esmall = w->esmall;
  if (ahead) {
    at = w->ahead.begin();
    rhat = (u64*)(w->ahead_block + (size_t)at.slot * w->ahead_set_bytes);
    esmall = (i64*)(w->ahead_block + (size_t)at.slot * w->ahead_set_bytes + w->ahead_rhat_bytes);
  }
  PrologueBatch pb{};
  ws_public(w, rhat, ahead ? w->ahead_set_bytes : w->rhat_bytes);   // r-hat of this encrypt
  PVW_TRY(fill_encrypt_jobs(c, pb, 0, ex, d_scalars, rhat, d_c1, d_c2));
  keys.fill(pb, 1);
  const i64 *es1 = nullptr, *es2 = nullptr;
  if (compact) {
    if (ex.r) {
      es1 = pb.job[1].explicit_coeffs;
      es2 = pb.job[2].explicit_coeffs;
      pb.njobs = 1;                                   // r only
    } else {
      pb.job[1].raw_out = esmall;
      pb.job[2].raw_out = esmall + (size_t)rA * l;
      es1 = pb.job[1].raw_out;
      es2 = pb.job[2].raw_out;
      pb.njobs = 3;
    }
  } else {
    pb.njobs = 3;
  }
  if (ahead) {
    pb.job[2].scalars = nullptr;                         // sampled only (raw_out): the MAC adds m g-hat, nothing of the caller's is read
    if (at.record_first) PVW_HIP(hipEventRecord(w->ahead_guard[at.bank], s));
    if (at.wait_guard) PVW_HIP(hipStreamWaitEvent(w->aux, w->ahead_guard[at.bank], 0));   // the MACs that read this bank last time round
    {
      ProfScope ps(c, "prologue_ahead", w->aux);
      PVW_HIP(launch_prologue(pb, c->dt, L, l, w->aux));
    }
    PVW_HIP(hipEventRecord(w->ahead_done[at.slot], w->aux));
    if (!ahead_host_wait(w->ahead_done[at.slot])) PVW_HIP(hipStreamWaitEvent(s, w->ahead_done[at.slot], 0));   // correct, as slow as in order
  } else {
    ProfScope ps(c, "prologue", s);
    PVW_HIP(launch_prologue(pb, c->dt, L, l, s));
  }
  {
    ProfScope ps(c, "mac_rows", s);
    MacSection a(width ? c->pkA : c->dA, compact ? nullptr : d_c1, out_c1, rA), b(width ? c->pkB : c->dB, compact ? nullptr : d_c2, out_c2, rB);
    if (compact) {
      a.e_small = es1;
      b.e_small = es2;
      b.scalars = d_scalars + c->party_lo;
    }
    if (RndState* rs = keys.state()) {
      a.rnd_ctr = &rs->counter;                          // the prologue in front of this launch was the state's reader
      a.rnd_adv = 1;
    }
    if (width) PVW_HIP(launch_mac_rows_packed(a, b, rhat, c->dt, k, L, l, width, s));   // the same sums over the packed copy
    else PVW_HIP(launch_mac_rows(a, b, rhat, c->dt, k, L, l, s));                       // crs.rs:188-201, encryption.rs:177-200
  }
  if (mark) {                                            // one record: the bank's guard where it is due, else the mark
    w->ahead_last = ahead && w->ahead.finish(at.slot) ? w->ahead_guard[at.bank] : w->ahead_mark;
    PVW_HIP(hipEventRecord(w->ahead_last, s));
  } else if (can_ahead) {
    w->ahead_last = nullptr;                             // (a call of another kind leaves the latest mark as it is)
  }
  if (out_repr == PVW_REPR_POWER) {
    ProfScope ps(c, "intt", s);
    PVW_HIP(launch_ntt(d_c1, rA, true, c->dt, L, l, s));
    PVW_HIP(launch_ntt(d_c2, rB, true, c->dt, L, l, s));
  }
  return PVW_OK;
}

// NOTE (measured): the prologue of call i under the MAC of call i-1, three times.
// Round 1: on a second stream with cross-stream event dependencies both ways -- step 242 us against 207 us in order at config 3.
// Round 3: with nothing but the seed feeding the prologue (compact addends), two sets of (r-hat, addends) and one device-side
// wait per stream and call: the prologue does run under the previous MAC (26 us there instead of 11), but the MAC behind the
// cross-stream wait starts as late as it did behind the prologue: step = MAC + 7.6-7.9 us against MAC + 7.8-8.3 us in order.
// Round 9 (profiles/r09_prologue_ahead_ab.txt), kept: the same two sets, but the HOST waits for the prologue and then enqueues
// the MAC with nothing in front of it.  Alternating processes on one box, bench.py, 9 + 9 at config 3: step - MAC 10.4-12.4 us
// at the parent, 3.2-6.3 us with the ahead path; the MAC itself runs 1-2.5 us longer with a prologue beside it, so the step
// goes 192.7-193.7 -> 186.8-188.1 us where mac_rows takes 181-184 us and 187.8 -> 183.8 us where it takes 175-178 us; at
// n = 1024 step - MAC 7.3-11.2 -> -0.5-1.9 us (66.7-70.9 -> 62.5-64.0 us).  What is left between two MACs is the kernel
// boundary, one unfenced event record and the slower MAC.

// The two single-dealer frames.  rnd: the seed forms' argument, NULL in the _rs forms (a seed form's NULL rnd is not a "NULL
// argument": encrypt_checks names it, behind the representation check).
static int32_t encrypt_device(pvw_ctx* c, const uint64_t* d_scalars, size_t num_scalars, const pvw_randomness_t* rnd,
                              const DealerKeys& keys, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  if (!c || !d_scalars || (keys.by_state && keys.missing()) || (!d_c1 && c->rowsA()) || (!d_c2 && c->rowsB()))
    return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_checks(c, num_scalars, rnd, keys, out_repr));
  return device_call(c, stream, [&](hipStream_t) { return keys.checks(c); }, [&](Workspace* w, hipStream_t s) {
    return encrypt_enqueue(c, w, d_scalars, keys, ExplicitRnd::of(rnd), d_c1, d_c2, out_repr, s);
  });
}

// host buffers: the scalars, and explicit randomness as global arrays, staged on the device
static int32_t encrypt_host(pvw_ctx* c, const uint64_t* scalars, size_t num_scalars, const pvw_randomness_t* rnd,
                            const DealerKeys& keys, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  if (!c || !scalars || (keys.by_state && keys.missing()) || !c1_out || !c2_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_checks(c, num_scalars, rnd, keys, out_repr));
  PVW_TRY(ensure_device(c));
  PVW_TRY(keys.checks(c));
  const size_t l = c->l, k = c->k, P = c->poly();
  // Output buffers the device can write (pvw_host_alloc, or memory the caller pinned / registered): the MAC stores c1 / c2
  // straight into them, 64 bytes per (row, limb) as its workgroups finish -- the 4.7 MB of config 3 cross PCIe under the
  // kernel instead of after it.  Pageable buffers take the copy.
  u64 *dir1 = nullptr, *dir2 = nullptr;
  if (out_repr == PVW_REPR_NTT) {
    dir1 = (u64*)device_alias(c1_out, k * P * 8);
    dir2 = (u64*)device_alias(c2_out, (size_t)c->n * P * 8);
    if (!dir1 || !dir2) dir1 = dir2 = nullptr;
  }
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_host_buffers(c, w));
    ExplicitRnd ex = ExplicitRnd::of(rnd);
    if (ex.r) {
      PVW_TRY(ws_scratch(w, (2 * k + c->n) * l * 8));
      i64* base = (i64*)w->scratch;
      PVW_HIP(hipMemcpyAsync(base, ex.r, k * l * 8, hipMemcpyHostToDevice, w->stream));
      PVW_HIP(hipMemcpyAsync(base + k * l, ex.e1, k * l * 8, hipMemcpyHostToDevice, w->stream));
      PVW_HIP(hipMemcpyAsync(base + 2 * k * l, ex.e2, (size_t)c->n * l * 8, hipMemcpyHostToDevice, w->stream));
      ex = ExplicitRnd{base, base + k * l, base + 2 * k * l};
    }
    PVW_HIP(hipMemcpyAsync(w->scalars, scalars, (size_t)c->n * 8, hipMemcpyHostToDevice, w->stream));
    PVW_TRY(encrypt_enqueue(c, w, w->scalars, keys, ex, w->c1, w->c2, out_repr, w->stream, dir1 ? dir1 + (size_t)c->c1_lo * P : nullptr,
                            dir2 ? dir2 + (size_t)c->party_lo * P : nullptr));
    if (!dir1) {
      PVW_HIP(hipMemcpyAsync(c1_out + (size_t)c->c1_lo * P, w->c1, (size_t)c->rowsA() * P * 8, hipMemcpyDeviceToHost, w->stream));
      PVW_HIP(hipMemcpyAsync(c2_out + (size_t)c->party_lo * P, w->c2, (size_t)c->rowsB() * P * 8, hipMemcpyDeviceToHost, w->stream));
    }
    return PVW_OK;
  });
}

// The exports of one operation differ in their key source alone.  Every frame runs in this order, which the tests hold it to:
// NULL arguments (the handle for NULL only), the argument checks, ensure_device, DealerKeys::checks (the first read of a
// handle), then the workspace and the stream.
int32_t pvw_encrypt_device(pvw_ctx* c, const uint64_t* d_scalars, size_t num_scalars, const pvw_randomness_t* rnd,
                           uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return encrypt_device(c, d_scalars, num_scalars, rnd, seed_of(rnd), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_encrypt_rs_device(pvw_ctx* c, const uint64_t* d_scalars, size_t num_scalars, void* handle, uint64_t* d_c1,
                              uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return encrypt_device(c, d_scalars, num_scalars, nullptr, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_encrypt(pvw_ctx* c, const uint64_t* scalars, size_t num_scalars, const pvw_randomness_t* rnd,
                    uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return encrypt_host(c, scalars, num_scalars, rnd, seed_of(rnd), c1_out, c2_out, out_repr);
}
int32_t pvw_encrypt_rs(pvw_ctx* c, const uint64_t* scalars, size_t num_scalars, void* handle, uint64_t* c1_out,
                       uint64_t* c2_out, uint32_t out_repr) {
  return encrypt_host(c, scalars, num_scalars, nullptr, DealerKeys::state(handle), c1_out, c2_out, out_repr);
}

// ------------------------------------------------------------------------ Shamir shares
// f_d(x) = s_d + a_{d,1} x + ... + a_{d,t} x^t over Z_p, party i gets f_d(i + 1).  The reference has no sharing code (its
// examples fill the share matrix with arbitrary numbers, examples/pvw.rs:95-131): the contract is this library's own.
static Mod shamir_mod(u64 p) {
  Mod m = make_mod(p);
  if (p == 2) { m.ratio_lo = 0; m.ratio_hi = (u64)1 << 63; }   // make_mod's quotient is one short for a power of two
  return m;
}
static int32_t shamir_modulus_check(u64 p) {
  if (p >= ((u64)1 << 62)) return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be below 2^62");
  if (!is_prime_u64(p)) return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be prime (Shamir shares live in a field)");
  return PVW_OK;
}
// The rules of a sharing, each stated once and worded for the entry point they serve.  pack != NULL is a packed call (DESIGN
// 8.14, K = *pack secrets per dealer at the points 0, -1, ..., -(K-1)); an unpacked call obeys the rules of K = 1.  The points
// 1..n and p-K+1..p-1, 0 must be distinct: p >= n + K; and K + degree values fix the polynomial: degree + K <= n.
static int32_t shamir_checks(const pvw_ctx* c, size_t D, uint32_t degree, u64 p, const uint32_t* pack = nullptr) {
  const u64 K = pack ? *pack : 1;
  if (D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no dealers");
  if (K == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at least 1");
  if (p < c->n + K)
    return fail(PVW_ERR_INVALID_PARAMETERS,
                pack ? "plain_modulus must be at least n + pack (evaluation points 1..n, secrets at 0..-(pack-1))"
                     : "plain_modulus must exceed the party count (evaluation points 1..n)");
  PVW_TRY(shamir_modulus_check(p));
  if (degree + K > c->n) {
    char buf[112];
    if (pack) snprintf(buf, sizeof buf, "degree %u with pack %u needs more than %u parties", degree, *pack, c->n);
    else snprintf(buf, sizeof buf, "degree %u needs more than %u parties", degree, c->n);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  return PVW_OK;
}

// the contract in plain C++ (no GPU): sequential draws, Horner.  Writes all n columns, whatever the context's shard.
int32_t pvw_shamir_shares_host(const pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                               uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  if (!c || !secrets || !shares_out || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(shamir_checks(c, num_dealers, degree, plain_modulus));
  const Mod m = shamir_mod(plain_modulus);
  const u32 n = c->n, t = degree;
  std::vector<u64> a((size_t)t + 1);
  for (size_t d = 0; d < num_dealers; ++d) {
    a[0] = reduce_word(secrets[d], m);
    for (u32 j = 1; j <= t; ++j) {
      if (coeffs) {
        a[j] = reduce_word(coeffs[d * t + (j - 1)], m);
      } else {
        ChaChaRng g;
        g.init(make_key(seeds + d * 32), PVW_DOM_SHAMIR, j);
        u64* o = &a[j];
        sample_residues_poly(g, 1, m.q, [o](u32, u64 v) { *o = v; });
      }
    }
    for (u32 i = 0; i < n; ++i) {
      const u64 x = (u64)i + 1;
      u64 acc = a[t];
      for (u32 j = t; j-- > 0;) acc = addmod(mulmod(acc, x, m), a[j], m.q);
      shares_out[d * n + i] = acc;
    }
  }
  volatile u64* va = a.data();                               // the coefficients are as secret as the secret
  for (size_t j = 0; j <= t; ++j) va[j] = 0;
  return PVW_OK;
}

// ------------------------------------------------------------------------ packed shares
// K = pack secrets per dealer at the points 0, -1, ..., -(K-1):
//   f_d(x) = sum_{j<K} s_{d,j} L_j(x) + Z(x) (a_{d,1} + a_{d,2} x + ... + a_{d,t} x^(t-1)),  Z(x) = x (x+1) ... (x+K-1)
// The points 1..n and p-K+1..p-1, 0 must be distinct: p >= n + K (shamir_checks).

// the contract in plain C++ (no GPU): L_j(x) and Z(x) from the definition with one inversion per denominator, sequential
// draws, Horner.  Writes all n columns, whatever the context's shard.
int32_t pvw_shamir_shares_packed_host(const pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                      uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  if (!c || !secrets || !shares_out || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(shamir_checks(c, num_dealers, degree, plain_modulus, &pack));
  const Mod m = shamir_mod(plain_modulus);
  const u32 n = c->n, t = degree, K = pack;
  // Lj[j * n + i] = L_j(i + 1) = prod_{m != j} (x + m) / (m - j), Z[i] = prod_m (x + m)
  std::vector<u64> Lj((size_t)K * n), Z(n), inv(K), suf((size_t)K + 1);
  for (u32 j = 0; j < K; ++j) {
    u64 den = 1;
    for (u32 mm = 0; mm < K; ++mm)
      if (mm != j) den = mulmod(den, submod((u64)mm, (u64)j, m.q), m);
    inv[j] = powmod(den, m.q - 2, m);
  }
  for (u32 i = 0; i < n; ++i) {
    const u64 x = (u64)i + 1;
    suf[K] = 1;                                                // suf[j] = prod_{m >= j}(x + m)
    for (u32 j = K; j-- > 0;) suf[j] = mulmod(suf[j + 1], x + j, m);
    Z[i] = suf[0];
    u64 pre = 1;                                               // prod_{m < j}(x + m)
    for (u32 j = 0; j < K; ++j) {
      Lj[(size_t)j * n + i] = mulmod(mulmod(pre, suf[j + 1], m), inv[j], m);
      pre = mulmod(pre, x + j, m);
    }
  }
  std::vector<u64> a((size_t)t + K);                           // s_{d,0..K-1} | a_{d,1..t}
  for (size_t d = 0; d < num_dealers; ++d) {
    for (u32 j = 0; j < K; ++j) a[j] = reduce_word(secrets[d * K + j], m);
    for (u32 j = 1; j <= t; ++j) {
      if (coeffs) {
        a[K + j - 1] = reduce_word(coeffs[d * t + (j - 1)], m);
      } else {
        ChaChaRng g;
        g.init(make_key(seeds + d * 32), PVW_DOM_SHAMIR, j);
        u64* o = &a[K + j - 1];
        sample_residues_poly(g, 1, m.q, [o](u32, u64 v) { *o = v; });
      }
    }
    for (u32 i = 0; i < n; ++i) {
      const u64 x = (u64)i + 1;
      u64 r = 0;                                               // a_1 + a_2 x + ... + a_t x^(t-1)
      for (u32 j = t; j-- > 0;) r = addmod(mulmod(r, x, m), a[K + j], m.q);
      u64 acc = mulmod(r, Z[i], m);
      for (u32 j = 0; j < K; ++j) acc = addmod(acc, mulmod(a[j], Lj[(size_t)j * n + i], m), m.q);
      shares_out[d * n + i] = acc;
    }
  }
  volatile u64* va = a.data();                               // the coefficients are as secret as the secrets
  for (size_t j = 0; j < a.size(); ++j) va[j] = 0;
  return PVW_OK;
}

// The rules every reconstruction's indices and modulus obey: distinct indices, points x_i = indices[i] + 1 below p, p a prime
// below 2^62.  The plain reconstruction (modulus_first) has always reported the modulus, then the range, then a duplicate; the
// checked and corrected calls a duplicate, then the range, then the modulus.
static int32_t shamir_index_checks(u64 p, const u64* indices, size_t count, bool modulus_first) {
  auto distinct = [&]() -> int32_t {
    std::vector<u64> sorted(indices, indices + count);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < count; ++i)
      if (sorted[i] == sorted[i - 1]) return fail(PVW_ERR_INVALID_PARAMETERS, "duplicate party index");
    return PVW_OK;
  };
  if (!modulus_first) PVW_TRY(distinct());
  if (p < 2) return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be prime (Shamir shares live in a field)");
  if (modulus_first) PVW_TRY(shamir_modulus_check(p));
  for (size_t i = 0; i < count; ++i)
    if (indices[i] >= p - 1) return fail(PVW_ERR_INVALID_PARAMETERS, "party index out of range for plain_modulus");
  return modulus_first ? distinct() : shamir_modulus_check(p);
}

// Lagrange weights at 0 for the points x_i = indices[i] + 1 (residues in [0, p)), behind the argument rules both callers share
static int32_t shamir_weights_at_zero(uint64_t plain_modulus, const uint64_t* indices, size_t count, Mod* mod, std::vector<u64>* wout) {
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares to reconstruct from");
  PVW_TRY(shamir_index_checks(plain_modulus, indices, count, true));
  const Mod m = shamir_mod(plain_modulus);
  // w_i = prod_{j != i} x_j / (x_j - x_i)
  std::vector<u64> w(count);
  for (size_t i = 0; i < count; ++i) {
    const u64 xi = indices[i] + 1;
    u64 num = 1, den = 1;
    for (size_t j = 0; j < count; ++j) {
      if (j == i) continue;
      const u64 xj = indices[j] + 1;
      num = mulmod(num, xj, m);
      den = mulmod(den, submod(xj, xi, m.q), m);
    }
    w[i] = mulmod(num, powmod(den, m.q - 2, m), m);
  }
  *mod = m;
  wout->swap(w);
  return PVW_OK;
}
// W[j][i] = the Lagrange weight AT the point z[j] (a residue) of x_i = indices[i] + 1 among the count points, in [0, p):
// u_i = (prod_{k != i}(x_i - x_k))^-1 once per source point (the barycentric weights), then per target
// u_i prod_{k != i}(z_j - x_k) from prefix and suffix products.  z_j = x_i gives the unit vector by itself.
static void shamir_weights_at_points(const Mod& m, const u64* indices, size_t count, const std::vector<u64>& z, std::vector<u64>* Wout) {
  std::vector<u64> u(count), W(z.size() * count), suf(count + 1);
  for (size_t i = 0; i < count; ++i) {
    u64 den = 1;
    for (size_t k = 0; k < count; ++k)
      if (k != i) den = mulmod(den, submod(indices[i] + 1, indices[k] + 1, m.q), m);
    u[i] = powmod(den, m.q - 2, m);
  }
  for (size_t j = 0; j < z.size(); ++j) {
    suf[count] = 1;                                            // suf[i] = prod_{k >= i}(z - x_k)
    for (size_t i = count; i-- > 0;) suf[i] = mulmod(suf[i + 1], submod(z[j], indices[i] + 1, m.q), m);
    u64 pre = 1;                                               // prod_{k < i}(z - x_k)
    for (size_t i = 0; i < count; ++i) {
      W[j * count + i] = mulmod(mulmod(pre, suf[i + 1], m), u[i], m);
      pre = mulmod(pre, submod(z[j], indices[i] + 1, m.q), m);
    }
  }
  Wout->swap(W);
}
// the residue w in [0, q) centred in (-q/2, q/2]
static i64 centred(u64 w, u64 q) { return w > q / 2 ? -(i64)(q - w) : (i64)w; }
// The weights once; then one dot product per secret.  Host only.
int32_t pvw_shamir_reconstruct(uint64_t plain_modulus, const uint64_t* indices, const uint64_t* shares, size_t count,
                               size_t num_secrets, uint64_t* out) {
  if (!indices || !shares || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Mod m;
  std::vector<u64> w;
  PVW_TRY(shamir_weights_at_zero(plain_modulus, indices, count, &m, &w));
  for (size_t sidx = 0; sidx < num_secrets; ++sidx) {
    u64 acc = 0;
    for (size_t i = 0; i < count; ++i) acc = addmod(acc, mulmod(reduce_word(shares[sidx * count + i], m), w[i], m), m.q);
    out[sidx] = acc;
  }
  return PVW_OK;
}
// The same weights for a caller that combines ciphertexts with them: centred in (-p/2, p/2], so that the noise
// of the combination grows by |w| and not by p - |w|.  Host only.
int32_t pvw_shamir_lagrange_weights(uint64_t plain_modulus, const uint64_t* indices, size_t count, int64_t* weights_out) {
  if (!indices || !weights_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Mod m;
  std::vector<u64> w;
  PVW_TRY(shamir_weights_at_zero(plain_modulus, indices, count, &m, &w));
  for (size_t i = 0; i < count; ++i) weights_out[i] = centred(w[i], m.q);
  return PVW_OK;
}
// The weights AT any points: row j for the point (targets[j] + 1) mod p -- p - 1 is the point 0, p - 1 - m the point
// -m of a packed sharing's secret m.  Host only.
int32_t pvw_shamir_lagrange_weights_at(uint64_t plain_modulus, const uint64_t* indices, size_t count, const uint64_t* targets,
                                       size_t num_targets, int64_t* weights_out) {
  if (!indices || !targets || !weights_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares to reconstruct from");
  if (num_targets == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no target points");
  PVW_TRY(shamir_index_checks(plain_modulus, indices, count, true));
  for (size_t j = 0; j < num_targets; ++j)
    if (targets[j] >= plain_modulus) return fail(PVW_ERR_INVALID_PARAMETERS, "target index out of range for plain_modulus");
  const Mod m = shamir_mod(plain_modulus);
  std::vector<u64> z(num_targets), W;
  for (size_t j = 0; j < num_targets; ++j) z[j] = targets[j] + 1 == m.q ? 0 : targets[j] + 1;
  shamir_weights_at_points(m, indices, count, z, &W);
  for (size_t i = 0; i < num_targets * count; ++i) weights_out[i] = centred(W[i], m.q);
  return PVW_OK;
}

// The way back of a packed sharing: out[s][j] = F_s(-j), j < pack, for the polynomial F_s through the count
// shares of row s; the Lagrange weights of the points indices[i] + 1 at each of 0, -1, ..., -(pack-1) once, then pack dot
// products per row.  The rules of pvw_shamir_reconstruct, and every index below p - pack (a point may not be a secret's).
int32_t pvw_shamir_reconstruct_packed(uint64_t plain_modulus, uint32_t pack, const uint64_t* indices, const uint64_t* shares, size_t count,
                                      size_t num_rows, uint64_t* out) {
  if (!indices || !shares || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (pack == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at least 1");
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares to reconstruct from");
  PVW_TRY(shamir_index_checks(plain_modulus, indices, count, true));
  for (size_t i = 0; i < count; ++i)
    if (plain_modulus < pack || indices[i] >= plain_modulus - pack)
      return fail(PVW_ERR_INVALID_PARAMETERS, "party index out of range for plain_modulus and pack");
  const Mod m = shamir_mod(plain_modulus);
  std::vector<u64> z(pack), W;
  for (u32 j = 0; j < pack; ++j) z[j] = j ? m.q - j : 0;
  shamir_weights_at_points(m, indices, count, z, &W);
  for (size_t r = 0; r < num_rows; ++r)
    for (u32 j = 0; j < pack; ++j) {
      u64 acc = 0;
      for (size_t i = 0; i < count; ++i)
        acc = addmod(acc, mulmod(reduce_word(shares[r * count + i], m), W[(size_t)j * count + i], m), m.q);
      out[r * pack + j] = acc;
    }
  return PVW_OK;
}

// ------------------------------------------------------------------------ checked reconstruction
// The basis columns 0..t give F_s; out[s] = F_s(0); every extra column is compared with F_s at its point.
// Reconstruct<F>, the layouts and the sizing rules: pvw_shamir_fields.h.  Its fields take their word counts from the kernels' header,
inline size_t NarrowField::interp_words(size_t count, u32 t) { return shamir_interp_words(count, t); }
inline size_t NarrowField::correct_public_words(size_t count, u32 t, size_t nk) { return shamir_correct_public_words(count, t, nk); }
inline size_t NarrowField::evaluate_public_words(size_t count, size_t Tg, size_t nk) { return shamir_evaluate_public_words(count, Tg, nk); }
inline size_t WideField::interp_words(size_t count, u32 t) { return shamir_interp_wide_words(count, t); }
inline size_t WideField::correct_public_words(size_t count, u32 t, size_t nk) { return shamir_correct_wide_public_words(count, t, nk); }
inline size_t WideField::evaluate_public_words(size_t count, size_t Tg, size_t nk) { return shamir_evaluate_wide_public_words(count, Tg, nk); }

// ... and a driver below takes from NarrowCalls or WideCalls everything else the two families differ in: the modulus as the kernels
// take it, their parameter blocks and launchers, the blocks of the stream's workspace, the locator bound, the names the timing
// tools look the ProfScopes up by, the messages, and the plain-C++ decoder the erasure host form runs on a sub-row.
struct NarrowCalls;
struct WideCalls;
// Where the evaluation points of a call come from: global party indices (the point is index + 1), field elements
// below p of four HOST words each (wide fields only), or the secret points 0, -1, ..., -(K - 1) of a packed wide sharing, which
// need no array.  F::target_points(t, j0, tg, ...) puts group j0 .. j0 + tg of them into the workspace.
struct EvalTargets {
  enum Kind { kIndices, kWidePoints, kPackedSecrets } kind;
  const u64* data;
  static EvalTargets indices(const u64* t) { return EvalTargets{kIndices, t}; }
  static EvalTargets wide_points(const u64* pts) { return EvalTargets{kWidePoints, pts}; }
  static EvalTargets packed_secrets() { return EvalTargets{kPackedSecrets, nullptr}; }
};
static void berlekamp_welch_host(const Reconstruct<NarrowCalls>& r, const uint64_t* shares, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                 uint64_t* err_mask, const uint64_t* targets, size_t num_targets, uint64_t* values);
static void berlekamp_welch_wide_host(const Reconstruct<WideCalls>& r, const uint64_t* shares, uint64_t* out, uint32_t* nerr,
                                      uint32_t* col_err, uint64_t* err_mask, const uint64_t* targets, size_t num_targets, uint64_t* values);
struct NarrowCalls : NarrowField {
  typedef Mod KMod;
  static KMod kmod(u64 p) { return shamir_mod(p); }
  typedef ShamirInterp Interp;
  typedef ShamirMatmul Matmul;
  typedef ShamirMaskedMatmul MaskedMatmul;
  typedef ShamirFinish Finish;
  typedef ShamirEvalFinish EvalFinish;
  static constexpr u64* Workspace::*interp = &Workspace::interp;
  static constexpr size_t Workspace::*interp_bytes = &Workspace::interp_bytes;
  static constexpr u64* Workspace::*correct = &Workspace::correct;
  static constexpr size_t Workspace::*correct_bytes = &Workspace::correct_bytes;
  static constexpr int kMaxLocator = PVW_SHAMIR_MAX_LOCATOR;
  static constexpr const char* kLocatorBound = "on the device the locator holds at most %d coefficients: count - degree - 1 must be below %d";
  static constexpr const char* kLayoutBound = "evaluation scratch: layout beyond its bound";
  static constexpr const char *kWeights = "shamir_weights", *kInterp = "shamir_interp", *kCorrectWeights = "shamir_correct_weights",
                              *kCorrect = "shamir_correct", *kEvaluate = "shamir_evaluate", *kEvaluateWeights = "shamir_evaluate_weights";
  // the launchers; launch_shamir_points takes no modulus, and the evaluate finish names the locator's values LamT / LamD
  static hipError_t points(const u64* idx, size_t n, u64* x, const KMod&, hipStream_t s) { return launch_shamir_points(idx, n, x, s); }
  static hipError_t target_points(const EvalTargets& t, size_t j0, size_t tg, u64* x, const KMod& m, hipStream_t s) {
    return points(t.data + j0, tg, x, m, s);               // the one-word family keeps indices only
  }
  static constexpr auto weights = &launch_shamir_weights;
  static constexpr auto interpolate = &launch_shamir_interp;
  static constexpr auto correct_weights = &launch_shamir_correct_weights;
  static constexpr auto matmul = &launch_shamir_matmul;
  static constexpr auto matmul_masked = &launch_shamir_matmul_masked;
  static constexpr auto bm = &launch_shamir_bm;
  static constexpr auto bm_erasures = &launch_shamir_bm_erasures;
  static constexpr auto correct_finish = &launch_shamir_correct_finish;
  static constexpr auto erasures_finish = &launch_shamir_erasures_finish;
  static constexpr auto ym = &launch_shamir_ym;
  static constexpr auto evaluate_weights = &launch_shamir_evaluate_weights;
  static hipError_t evaluate_finish(EvalFinish& f, const u64* lamT, const u64* lamD, hipStream_t s) {
    f.LamT = lamT, f.LamD = lamD;
    return launch_shamir_evaluate_finish(f, s);
  }
  static constexpr auto decode = &berlekamp_welch_host;
};
struct WideCalls : WideField {
  typedef WideMont KMod;
  static KMod kmod(const u64* p) { return make_wide_mont(p); }
  typedef ShamirInterpWide Interp;
  typedef ShamirMatmulWide Matmul;
  typedef ShamirMaskedMatmulWide MaskedMatmul;
  typedef ShamirFinishWide Finish;
  typedef ShamirEvalFinishWide EvalFinish;
  static constexpr u64* Workspace::*interp = &Workspace::interp_wide;
  static constexpr size_t Workspace::*interp_bytes = &Workspace::interp_wide_bytes;
  static constexpr u64* Workspace::*correct = &Workspace::correct_wide;
  static constexpr size_t Workspace::*correct_bytes = &Workspace::correct_wide_bytes;
  // with a mask as well: r + 3 elements of LDS then, 131 136 bytes at the bound
  static constexpr int kMaxLocator = PVW_SHAMIR_WIDE_MAX_LOCATOR;
  static constexpr const char* kLocatorBound = "on the device the wide locator holds at most %d coefficients: count - degree - 1 must be below %d";
  static constexpr const char* kLayoutBound = "wide evaluation scratch: layout beyond its bound";
  static constexpr const char *kWeights = "shamir_weights_wide", *kInterp = "shamir_interp_wide", *kCorrectWeights = "shamir_correct_wide_weights",
                              *kCorrect = "shamir_correct_wide", *kEvaluate = "shamir_evaluate_wide",
                              *kEvaluateWeights = "shamir_evaluate_wide_weights";
  // the launchers; the evaluate finish names the locator's values PsiT / PsiD
  static constexpr auto points = &launch_shamir_points_wide;
  static hipError_t target_points(const EvalTargets& t, size_t j0, size_t tg, u64* x, const KMod& m, hipStream_t s) {
    switch (t.kind) {
      case EvalTargets::kWidePoints: return launch_shamir_points_from_wide(t.data + j0 * 4, tg, x, m, s);
      case EvalTargets::kPackedSecrets: return launch_shamir_packed_secret_points_wide((u32)j0, tg, x, m, s);
      default: return launch_shamir_points_wide(t.data + j0, tg, x, m, s);
    }
  }
  static constexpr auto weights = &launch_shamir_weights_wide;
  static constexpr auto interpolate = &launch_shamir_interp_wide;
  static constexpr auto correct_weights = &launch_shamir_correct_weights_wide;
  static constexpr auto matmul = &launch_shamir_matmul_wide;
  static constexpr auto matmul_masked = &launch_shamir_matmul_masked_wide;
  static constexpr auto bm = &launch_shamir_bm_wide;
  static constexpr auto bm_erasures = &launch_shamir_bm_erasures_wide;
  static constexpr auto correct_finish = &launch_shamir_correct_finish_wide;
  static constexpr auto erasures_finish = &launch_shamir_erasures_finish_wide;
  static constexpr auto ym = &launch_shamir_ym_wide;
  static constexpr auto evaluate_weights = &launch_shamir_evaluate_weights_wide;
  static hipError_t evaluate_finish(EvalFinish& f, const u64* psiT, const u64* psiD, hipStream_t s) {
    f.PsiT = psiT, f.PsiD = psiD;
    return launch_shamir_evaluate_finish_wide(f, s);
  }
  static constexpr auto decode = &berlekamp_welch_wide_host;
};

extern "C++" {
// What the argument checks of both fields begin with, in this order: NULL (`given`: every pointer of the call is there), no
// secrets, too few shares.  reconstruct_checks and reconstruct_wide_checks go on from here, each by its own index rules.
template <class F>
static int32_t reconstruct_front_checks(const Reconstruct<F>& r, bool given) {
  if (!given) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (r.S == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no secrets to reconstruct");
  if (r.count < (size_t)r.degree + 1) {
    char buf[96];
    snprintf(buf, sizeof buf, "degree %u needs at least %zu shares, got %zu", r.degree, (size_t)r.degree + 1, r.count);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  return PVW_OK;
}
static int32_t reconstruct_checks(const Reconstruct<NarrowCalls>& r, const void* shares, const void* out) {
  PVW_TRY(reconstruct_front_checks(r, r.indices && shares && out));
  PVW_TRY(shamir_index_checks(r.p, r.indices, r.count, false));
  if (r.secret_stride == 0 || r.point_stride == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a stride of 0");
  return PVW_OK;
}
// what the kernels' 32-bit counts hold (the host routine has no such bound)
template <class F>
static int32_t reconstruct_device_checks(const Reconstruct<F>& r) {
  if (r.count >= ((size_t)1 << 31) || r.S >= ((size_t)1 << 31))
    return fail(PVW_ERR_INVALID_PARAMETERS, "count and num_secrets must be below 2^31 on the device");
  return PVW_OK;
}
}  // extern "C++"

// The contract in plain C++ (no GPU), written apart from the kernels' barycentric form: for every target the basis
// polynomials L_j(x) = prod_{i != j}(x - x_i) / prod_{i != j}(x_j - x_i) are evaluated directly, then one dot product per secret.
int32_t pvw_shamir_reconstruct_checked_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                            const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                            uint64_t* out, uint32_t* bad, uint32_t* col_bad) {
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, shares, out));
  const Mod m = shamir_mod(plain_modulus);
  const size_t t = degree, T = r.T();
  std::vector<u64> x(count), inv_den(t + 1), L(t + 1);
  for (size_t c = 0; c < count; ++c) x[c] = indices[c] + 1;
  for (size_t j = 0; j <= t; ++j) {
    u64 den = 1;
    for (size_t i = 0; i <= t; ++i)
      if (i != j) den = mulmod(den, submod(x[j], x[i], m.q), m);
    inv_den[j] = powmod(den, m.q - 2, m);
  }
  if (bad) std::fill(bad, bad + num_secrets, 0u);
  if (col_bad) std::fill(col_bad, col_bad + count, 0u);
  for (size_t tm = 0; tm < T; ++tm) {
    const u64 xm = tm ? x[t + tm] : 0;
    for (size_t j = 0; j <= t; ++j) {
      u64 num = 1;
      for (size_t i = 0; i <= t; ++i)
        if (i != j) num = mulmod(num, submod(xm, x[i], m.q), m);
      L[j] = mulmod(num, inv_den[j], m);
    }
    for (size_t s = 0; s < num_secrets; ++s) {
      const u64* row = shares + s * secret_stride;
      u64 v = 0;
      for (size_t j = 0; j <= t; ++j) v = addmod(v, mulmod(reduce_word(row[j * point_stride], m), L[j], m), m.q);
      if (tm == 0) {
        out[s] = v;
      } else if (reduce_word(row[(t + tm) * point_stride], m) != v) {
        if (bad) ++bad[s];
        if (col_bad) ++col_bad[t + tm];
      }
    }
  }
  return PVW_OK;
}

extern "C++" {
// the points and the weight matrix of one call into ws (F::interp_words words)
template <class F>
static int32_t reconstruct_weights(pvw_ctx* c, const Reconstruct<F>& r, const typename F::KMod& m, u64* ws, hipStream_t s) {
  ProfScope ps(c, F::kWeights, s);
  PVW_HIP(F::points(r.indices, r.count, ws, m, s));
  PVW_HIP(F::weights(ws, r.count, r.degree, m, s));
  return PVW_OK;
}
// ns secrets from d_shares under the weights in ws: out and bad of these secrets; col_bad, zeroed by the caller, is added to
template <class F>
static int32_t reconstruct_interp(pvw_ctx* c, const Reconstruct<F>& r, const typename F::KMod& m, const u64* ws, const u64* d_shares,
                                  size_t ns, size_t secret_stride, size_t point_stride, u64* d_out, u32* d_bad, u32* d_col_bad,
                                  hipStream_t s) {
  ProfScope ps(c, F::kInterp, s);
  PVW_HIP(launch_shamir_zero_counts(d_bad, ns, s));
  typename F::Interp b{};
  b.shares = d_shares;
  b.secret_stride = secret_stride;
  b.point_stride = point_stride;
  b.W = ws + (2 * r.count + 1) * F::EW;
  b.out = d_out;
  b.bad = d_bad;
  b.col_bad = d_col_bad;
  b.ns = (u32)ns;
  b.degree = r.degree;
  b.T = (u32)r.T();
  b.m = m;
  PVW_HIP(F::interpolate(b, s));
  return PVW_OK;
}

// Under stream capture a call may not allocate: the block of the stream's workspace that the call grows (`bytes`: interp_bytes
// or correct_bytes) must hold `need` already, which an earlier call of the same size outside capture leaves (checked before the
// workspace is looked up, like multi_capture_check, and refused with the same code and the caller's message)
static int32_t grown_capture_check(pvw_ctx* c, hipStream_t s, size_t Workspace::*bytes, size_t need, const char* msg) {
  if (!stream_capturing(s)) return PVW_OK;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = c->async_ws.find((void*)s);
  if (it != c->async_ws.end() && it->second->*bytes >= need) return PVW_OK;
  return fail(PVW_ERR_INVALID_PARAMETERS, msg);
}

// The checked device call behind its argument checks
template <class F>
static int32_t checked_device_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* d_shares, u64* d_out, u32* d_bad, u32* d_col_bad,
                                   void* stream) {
  const typename F::KMod m = F::kmod(r.p);
  // A context that has not touched its device yet initialises it inside device_call (allocations, a wait): on a capturing
  // stream that would invalidate the caller's capture, and nothing can have sized the workspace.  So the caller's stream is
  // checked before anything else; the context's own stream (stream == NULL) exists only once the device is initialised.
  auto sized = [&](hipStream_t s) {
    return grown_capture_check(c, s, F::interp_bytes, r.ws_bytes(),
                               "checked reconstruction under stream capture: run a call with the same degree and count on this stream "
                               "outside capture first (it sizes the workspace)");
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(ws_grow(&(w->*F::interp), &(w->*F::interp_bytes), r.ws_bytes(), s, false));   // public: nothing to clear
    PVW_TRY(reconstruct_weights(c, r, m, w->*F::interp, s));
    PVW_HIP(launch_shamir_zero_counts(d_col_bad, r.count, s));
    return reconstruct_interp(c, r, m, w->*F::interp, d_shares, r.S, r.secret_stride, r.point_stride, d_out, d_bad, d_col_bad, s);
  });
}
}  // extern "C++"

int32_t pvw_shamir_reconstruct_checked_device(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                              size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                              size_t point_stride, uint64_t* d_out, uint32_t* d_bad, uint32_t* d_col_bad, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, d_shares, d_out));
  PVW_TRY(reconstruct_device_checks(r));
  return checked_device_call(c, r, d_shares, d_out, d_bad, d_col_bad, stream);
}

extern "C++" {
// The staging of the host-buffer reconstruction calls of both fields (8.10 - 8.16, 8.19 - 8.22): the secrets go up in pieces of
// `per`, each as a dense [cnt][count][EW] block at d_sh -- whole rows by a 2D copy where the caller's rows lie that way, else
// repacked on the host --, and the stream is drained behind a piece before the next one reuses the staging.  piece(s0, cnt)
// enqueues the kernels of secrets [s0, s0 + cnt) and their downloads.  The host copy is as secret as the caller's shares: it is
// wiped when the call ends.
template <class F>
struct ShareStaging {
  static constexpr size_t EW = F::EW;
  const Reconstruct<F>& r;
  const u64* shares;
  size_t per;
  bool dense;                                                    // whole rows go up as they lie
  std::vector<u64> packed;                                       // a piece's shares when they do not
  ShareStaging(const Reconstruct<F>& r_, const u64* shares_, size_t per_)
      : r(r_), shares(shares_), per(per_), dense(r_.point_stride == 1 && r_.secret_stride >= r_.count) {
    if (!dense) packed.resize(per * r.count * EW);
  }
  ~ShareStaging() {
    volatile u64* vp = packed.data();
    for (size_t i = 0; i < packed.size(); ++i) vp[i] = 0;
  }
  // the rows [S][ewords] of the caller's erasure mask go up with their shares, dense as they lie, to d_erased
  const u64* erased = nullptr;
  u64* d_erased = nullptr;
  size_t ewords() const { return (r.count + 63) / 64; }
  int32_t run(u64* d_sh, hipStream_t stream, const std::function<int32_t(size_t s0, size_t cnt)>& piece) {
    const size_t count = r.count, row = count * EW * 8;
    for (size_t s0 = 0; s0 < r.S; s0 += per) {
      const size_t cnt = (r.S - s0) < per ? (r.S - s0) : per;
      if (erased) PVW_HIP(hipMemcpyAsync(d_erased, erased + s0 * ewords(), cnt * ewords() * 8, hipMemcpyHostToDevice, stream));
      if (dense) {
        PVW_HIP(hipMemcpy2DAsync(d_sh, row, shares + s0 * r.secret_stride * EW, r.secret_stride * EW * 8, row, cnt, hipMemcpyHostToDevice, stream));
      } else {
        for (size_t s = 0; s < cnt; ++s)
          for (size_t col = 0; col < count; ++col)
            memcpy(&packed[(s * count + col) * EW], shares + ((s0 + s) * r.secret_stride + col * r.point_stride) * EW, EW * 8);
        PVW_HIP(hipMemcpyAsync(d_sh, packed.data(), cnt * row, hipMemcpyHostToDevice, stream));
      }
      PVW_TRY(piece(s0, cnt));
      PVW_HIP(hipStreamSynchronize(stream));                     // the next piece reuses the staging
    }
    return PVW_OK;
  }
};

// host buffers: the secrets go up in pieces of `per` (<= ~1 GiB of shares), each packed to [piece][count]; the weights are
// made once.  The staged shares and the staged results are secret; the weights and the counts are not.
template <class F>
static int32_t checked_host_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* shares, u64* out, u32* bad, u32* col_bad) {
  PVW_TRY(ensure_device(c));
  constexpr size_t EB = F::EW * 8;                               // bytes per element
  const typename F::KMod m = F::kmod(r.p);
  const size_t count = r.count, per = chunk_1gib((count + 1) * EB + 4, r.S);
  Scratch sc;
  const size_t r_sh = sc.add(per * count * EB), r_out = sc.add(per * EB), r_ws = sc.add(r.ws_bytes()), r_bad = sc.add(per * 4),
               r_col = sc.add(count * 4);
  ShareStaging<F> st(r, shares, per);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    sc.secret(w, r_sh, r_out);
    u64 *d_sh = sc.at(r_sh), *d_out = sc.at(r_out), *ws = sc.at(r_ws);
    u32 *d_bad = bad ? sc.at<u32>(r_bad) : nullptr, *d_col = col_bad ? sc.at<u32>(r_col) : nullptr;
    PVW_TRY(reconstruct_weights(c, r, m, ws, w->stream));
    PVW_HIP(launch_shamir_zero_counts(d_col, count, w->stream));
    PVW_TRY(st.run(d_sh, w->stream, [&](size_t s0, size_t cnt) -> int32_t {
      PVW_TRY(reconstruct_interp(c, r, m, ws, d_sh, cnt, count, 1, d_out, d_bad, d_col, w->stream));
      PVW_HIP(hipMemcpyAsync(out + s0 * F::EW, d_out, cnt * EB, hipMemcpyDeviceToHost, w->stream));
      if (bad) PVW_HIP(hipMemcpyAsync(bad + s0, d_bad, cnt * 4, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    }));
    if (col_bad) PVW_HIP(hipMemcpyAsync(col_bad, d_col, count * 4, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}
}  // extern "C++"
int32_t pvw_shamir_reconstruct_checked(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                       const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                       uint64_t* out, uint32_t* bad, uint32_t* col_bad) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, shares, out));
  PVW_TRY(reconstruct_device_checks(r));
  return checked_host_call(c, r, shares, out, bad, col_bad);
}

// ------------------------------------------------------------------------ corrected reconstruction
// r = count - t - 1 redundant columns, E = r / 2: secret s is decodable iff some F_s of degree <= t disagrees with its row in at
// most E columns; F_s is then unique, out[s] = F_s(0) and the disagreeing columns are reported.  No column is a basis.

// The contract in plain C++ (no GPU), by another method than the kernels' (syndromes, Berlekamp-Massey, locator roots):
// Berlekamp-Welch.  Find N of degree <= t + E and a monic W of degree E with N(x_c) = y_c W(x_c) in every column, by Gaussian
// elimination on count equations in t + 2E + 1 unknowns; if F_s exists, every solution has N = F_s W.  So: no solution, W does
// not divide N, or N / W disagrees with more than E columns: undecodable.  Cubic in count per secret.
// With targets: values[s][j] = F_s(targets[j] + 1) by Horner over the quotient's coefficients, 0 for an undecodable row
// (pvw_shamir_evaluate_corrected_host); out may then be NULL.  The argument checks are the callers'.
static void berlekamp_welch_host(const Reconstruct<NarrowCalls>& r, const uint64_t* shares, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                 uint64_t* err_mask, const uint64_t* targets, size_t num_targets, uint64_t* values) {
  const uint64_t plain_modulus = r.p;
  const uint64_t* indices = r.indices;
  const size_t count = r.count, num_secrets = r.S, secret_stride = r.secret_stride, point_stride = r.point_stride;
  const uint32_t degree = r.degree;
  const Mod m = shamir_mod(plain_modulus);
  const size_t t = degree, E = (count - t - 1) / 2, nq = t + E + 1, nu = nq + E, words = (count + 63) / 64;
  std::vector<u64> x(count), y(count), A(count * (nu + 1)), sol(nu), W(E + 1), N(nq);
  std::vector<size_t> pivot_col;
  for (size_t c = 0; c < count; ++c) x[c] = indices[c] + 1;
  if (col_err) std::fill(col_err, col_err + count, 0u);
  for (size_t s = 0; s < num_secrets; ++s) {
    for (size_t c = 0; c < count; ++c) y[c] = reduce_word(shares[s * secret_stride + c * point_stride], m);
    // row c: sum_j N_j x^j - y sum_{k < E} W_k x^k = y x^E
    for (size_t c = 0; c < count; ++c) {
      u64* row = &A[c * (nu + 1)];
      u64 pw = 1;
      for (size_t j = 0; j < nq; ++j) {
        row[j] = pw;
        if (j < E) row[nq + j] = submod(0, mulmod(y[c], pw, m), m.q);
        if (j == E) row[nu] = mulmod(y[c], pw, m);
        pw = mulmod(pw, x[c], m);
      }
    }
    pivot_col.clear();
    size_t rank = 0;
    for (size_t col = 0; col < nu && rank < count; ++col) {
      size_t pr = rank;
      while (pr < count && A[pr * (nu + 1) + col] == 0) ++pr;
      if (pr == count) continue;
      if (pr != rank) std::swap_ranges(&A[pr * (nu + 1)], &A[(pr + 1) * (nu + 1)], &A[rank * (nu + 1)]);
      u64* prow = &A[rank * (nu + 1)];
      const u64 inv = powmod(prow[col], m.q - 2, m);
      for (size_t j = col; j <= nu; ++j) prow[j] = mulmod(prow[j], inv, m);
      for (size_t i = 0; i < count; ++i) {
        u64* row = &A[i * (nu + 1)];
        const u64 f = row[col];
        if (i == rank || f == 0) continue;
        for (size_t j = col; j <= nu; ++j) row[j] = submod(row[j], mulmod(f, prow[j], m), m.q);
      }
      pivot_col.push_back(col);
      ++rank;
    }
    bool ok = true;
    for (size_t i = rank; i < count && ok; ++i) ok = A[i * (nu + 1) + nu] == 0;   // a row 0 = b: no solution
    u64 secret = 0;
    std::vector<size_t> wrong;
    if (ok) {
      std::fill(sol.begin(), sol.end(), 0);                                      // free unknowns: 0
      for (size_t i = 0; i < rank; ++i) sol[pivot_col[i]] = A[i * (nu + 1) + nu];
      for (size_t j = 0; j < nq; ++j) N[j] = sol[j];
      for (size_t k = 0; k < E; ++k) W[k] = sol[nq + k];
      W[E] = 1;
      // N / W by long division (W monic): the quotient stays in N[E ..], the remainder in N[.. E)
      for (size_t i = nq; i-- > E;) {
        const u64 f = N[i];
        for (size_t k = 0; k < E; ++k) N[i - E + k] = submod(N[i - E + k], mulmod(f, W[k], m), m.q);
      }
      for (size_t k = 0; k < E && ok; ++k) ok = N[k] == 0;
      if (ok) {
        const u64* F = &N[E];                                                    // degree <= t
        for (size_t c = 0; c < count; ++c) {
          u64 v = F[t];
          for (size_t j = t; j-- > 0;) v = addmod(mulmod(v, x[c], m), F[j], m.q);
          if (v != y[c]) wrong.push_back(c);
        }
        ok = wrong.size() <= E;
        secret = F[0];
        for (size_t j = 0; j < num_targets && ok; ++j) {
          const u64 xs = targets[j] + 1;
          u64 v = F[t];
          for (size_t i = t; i-- > 0;) v = addmod(mulmod(v, xs, m), F[i], m.q);
          values[s * num_targets + j] = v;
        }
      }
    }
    if (!ok && values) std::fill(values + s * num_targets, values + (s + 1) * num_targets, (u64)0);
    if (out) out[s] = ok ? secret : 0;
    if (nerr) nerr[s] = ok ? (u32)wrong.size() : PVW_SHAMIR_UNDECODABLE;
    if (err_mask) std::fill(err_mask + s * words, err_mask + (s + 1) * words, (u64)0);
    if (ok)
      for (size_t c : wrong) {
        if (col_err) ++col_err[c];
        if (err_mask) err_mask[s * words + c / 64] |= (u64)1 << (c % 64);
      }
  }
  for (std::vector<u64>* v : {&y, &A, &sol, &W, &N}) {                           // as secret as the shares
    volatile u64* vp = v->data();
    for (size_t i = 0; i < v->size(); ++i) vp[i] = 0;
  }
}
int32_t pvw_shamir_reconstruct_corrected_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                              const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                              uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, shares, out));
  berlekamp_welch_host(r, shares, out, nerr, col_err, err_mask, nullptr, 0, nullptr);
  return PVW_OK;
}

extern "C++" {
// Secrets per pass and targets per group (correct_piece, evaluate_piece, evaluate_group) are sized within these budgets (tuning
// build: PVW_CORRECT_PIECE_BYTES and PVW_EVALUATE_GROUP_BYTES, read per call, so that the tests take several passes and walk
// several groups at small shapes)
static size_t piece_budget() {
  const long env = PVW_ENV_INT("PVW_CORRECT_PIECE_BYTES", 0);
  return env > 0 ? (size_t)env : (size_t)64 << 20;
}
static size_t group_budget() {
  const long env = PVW_ENV_INT("PVW_EVALUATE_GROUP_BYTES", 0);
  return env > 0 ? (size_t)env : (size_t)64 << 20;
}
template <class F>
static int32_t correct_device_checks(const Reconstruct<F>& r) {
  PVW_TRY(reconstruct_device_checks(r));
  if (r.red() / 2 + 1 > (size_t)F::kMaxLocator) {
    char buf[160];
    snprintf(buf, sizeof buf, F::kLocatorBound, F::kMaxLocator, 2 * F::kMaxLocator);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  return PVW_OK;
}
// the points and the public matrices of one call
template <class F>
static int32_t correct_weights(pvw_ctx* c, const Reconstruct<F>& r, const typename F::KMod& m, const CorrectLayout<F>& lay, u64* ws,
                               hipStream_t s) {
  ProfScope ps(c, F::kCorrectWeights, s);
  PVW_HIP(F::points(r.indices, r.count, ws + lay.pub, m, s));
  PVW_HIP(F::correct_weights(ws + lay.pub, r.count, r.degree, (u32)lay.nk, m, s));
  return PVW_OK;
}
// ns <= lay.cap secrets from d_shares: their out, nerr and mask rows; col_err, zeroed by the caller, is added to.
// d_erased: the ns rows of the erasure mask, or NULL for the calls without one.
template <class F>
static int32_t correct_piece_enqueue(pvw_ctx* c, const Reconstruct<F>& r, const typename F::KMod& m, const CorrectLayout<F>& lay, u64* ws,
                                     const u64* d_shares, size_t ns, size_t secret_stride, size_t point_stride, u64* d_out, u32* d_nerr,
                                     u32* d_col_err, u64* d_mask, hipStream_t s, const u64* d_erased) {
  ProfScope ps(c, F::kCorrect, s);
  constexpr size_t EW = F::EW;
  const u64* pub = ws + lay.pub;
  const u64 *lambda = pub + (2 * r.count + 1) * EW, *V = lambda + r.count * EW, *X = V + r.count * lay.r * EW;
  u64 *M = ws, *synd = ws + lay.synd, *Lam = ws + lay.lam;
  u32* L = (u32*)(ws + lay.L);
  typename F::MaskedMatmul a{};
  a.A = d_shares, a.secret_stride = secret_stride, a.term_stride = point_stride;
  a.W = V, a.out = synd;
  a.ns = (u32)ns, a.terms = (u32)r.count, a.T = (u32)lay.r, a.m = m;
  a.erased = d_erased, a.ewords = (u32)((r.count + 63) / 64);
  if (d_erased) {
    PVW_HIP(F::matmul_masked(a, s));
    PVW_HIP(F::bm_erasures(synd, d_erased, pub, Lam, L, (u32)ns, (u32)r.count, (u32)lay.r, m, s));
  } else {
    PVW_HIP(F::matmul(a, s));
    PVW_HIP(F::bm(synd, Lam, L, (u32)ns, (u32)lay.r, m, s));
  }
  typename F::Matmul b{};
  b.A = Lam, b.secret_stride = lay.nk, b.term_stride = 1;
  b.W = X, b.out = M;
  b.ns = (u32)ns, b.terms = (u32)lay.nk, b.T = (u32)r.count, b.m = m;
  PVW_HIP(F::matmul(b, s));
  typename F::Finish f{};
  f.shares = d_shares, f.secret_stride = secret_stride, f.point_stride = point_stride;
  f.M = M, f.Lam = Lam, f.L = L, f.lam = lambda;
  f.out = d_out, f.nerr = d_nerr, f.col_err = d_col_err, f.mask = d_mask;
  f.count = (u32)r.count, f.E = (u32)lay.nk - 1, f.m = m;
  if (d_erased) PVW_HIP(F::erasures_finish(f, d_erased, (u32)ns, s));
  else PVW_HIP(F::correct_finish(f, (u32)ns, s));
  return PVW_OK;
}

// The stream's `correct` block (F::correct) for a device call of the corrected decode or of the evaluation: grown to `need` bytes,
// and the regions (word offset, bytes) the call's secrets decide marked secret -- M, which leads the block, and for the evaluation
// y o M | raw | the stand-in for out.
template <class F>
static int32_t correct_block(Workspace* w, size_t need, std::initializer_list<std::pair<size_t, size_t>> secret, hipStream_t s) {
  if (w->*F::correct_bytes < need) ws_public(w, w->*F::correct, w->*F::correct_bytes);   // the block is about to go
  PVW_TRY(ws_grow(&(w->*F::correct), &(w->*F::correct_bytes), need, s, true));
  for (const auto& sp : secret) ws_mark_secret(w, w->*F::correct + sp.first, sp.second);
  return PVW_OK;
}
// ... and its passes over the kernels: pass(s0, ns) for every `cap` of the call's S secrets
static int32_t correct_passes(size_t S, size_t cap, const std::function<int32_t(size_t s0, size_t ns)>& pass) {
  for (size_t s0 = 0; s0 < S; s0 += cap) PVW_TRY(pass(s0, S - s0 < cap ? S - s0 : cap));
  return PVW_OK;
}

// The device call of 8.11 or 8.20 behind its argument checks; with d_erased (r.erasures) that of 8.16 or 8.21.  `unsized`: what a
// captured call is refused with when nothing has sized the workspace.
template <class F>
static int32_t corrected_device_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* d_shares, const u64* d_erased, u64* d_out, u32* d_nerr,
                                     u32* d_col_err, u64* d_err_mask, void* stream, const char* unsized) {
  constexpr size_t EW = F::EW;
  const typename F::KMod m = F::kmod(r.p);
  const CorrectLayout<F> lay(r, correct_piece(r, piece_budget()));
  const size_t words = (r.count + 63) / 64;
  // the caller's stream is checked before the context initialises its device (checked_device_call)
  auto sized = [&](hipStream_t s) { return grown_capture_check(c, s, F::correct_bytes, lay.bytes(), unsized); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(correct_block<F>(w, lay.bytes(), {{0, lay.m_bytes()}}, s));
    u64* ws = w->*F::correct;
    PVW_TRY(correct_weights(c, r, m, lay, ws, s));
    PVW_HIP(launch_shamir_zero_counts(d_col_err, r.count, s));
    return correct_passes(r.S, lay.cap, [&](size_t s0, size_t ns) {
      return correct_piece_enqueue(c, r, m, lay, ws, d_shares + s0 * r.secret_stride * EW, ns, r.secret_stride, r.point_stride,
                                   d_out + s0 * EW, Report::from(d_nerr, s0), d_col_err, Report::from(d_err_mask, s0 * words), s,
                                   Report::from(d_erased, s0 * words));
    });
  });
}

// host buffers: the secrets go up in pieces as the checked call stages them (ShareStaging: each packed to [piece][count][EW], or
// whole rows by a 2D copy), a piece no larger than one pass over the kernels; the public matrices are made once and col_err
// adds up over the pieces.  The staged shares, the staged secrets and M are cleared before the call returns.
// Behind the argument checks; with `erased` (r.erasures) the host-buffer call of 8.16 or 8.21, whose mask rows are staged with the
// shares of their piece.
template <class F>
static int32_t corrected_host_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* shares, const u64* erased, u64* out, u32* nerr,
                                   u32* col_err, u64* err_mask) {
  PVW_TRY(ensure_device(c));
  constexpr size_t EB = F::EW * 8;                               // bytes per element
  const typename F::KMod m = F::kmod(r.p);
  const size_t count = r.count, words = (count + 63) / 64;
  size_t per = chunk_1gib((count + 1) * EB + (words + (erased ? words : 0)) * 8 + 4, r.S);
  if (per > correct_piece(r, piece_budget())) per = correct_piece(r, piece_budget());
  const CorrectLayout<F> lay(r, per);
  Scratch sc;
  const size_t r_sh = sc.add(per * count * EB), r_out = sc.add(per * EB), r_ws = sc.add(lay.bytes()), r_nerr = sc.add(per * 4),
               r_col = sc.add(count * 4), r_mask = sc.add(per * words * 8), r_er = sc.add(erased ? per * words * 8 : 0);
  ShareStaging<F> st(r, shares, per);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    u64 *d_sh = sc.at(r_sh), *d_out = sc.at(r_out), *ws = sc.at(r_ws);
    ws_mark_secret(w, d_sh, (size_t)((char*)ws - (char*)d_sh) + lay.m_bytes());   // staged shares | staged secrets | M
    u32 *d_nerr = nerr ? sc.at<u32>(r_nerr) : nullptr, *d_col = col_err ? sc.at<u32>(r_col) : nullptr;
    u64* d_mask = err_mask ? sc.at(r_mask) : nullptr;
    if (erased) st.erased = erased, st.d_erased = sc.at(r_er);
    PVW_TRY(correct_weights(c, r, m, lay, ws, w->stream));
    PVW_HIP(launch_shamir_zero_counts(d_col, count, w->stream));
    PVW_TRY(st.run(d_sh, w->stream, [&](size_t s0, size_t cnt) -> int32_t {
      PVW_TRY(correct_piece_enqueue(c, r, m, lay, ws, d_sh, cnt, count, 1, d_out, d_nerr, d_col, d_mask, w->stream, st.d_erased));
      PVW_HIP(hipMemcpyAsync(out + s0 * F::EW, d_out, cnt * EB, hipMemcpyDeviceToHost, w->stream));
      if (nerr) PVW_HIP(hipMemcpyAsync(nerr + s0, d_nerr, cnt * 4, hipMemcpyDeviceToHost, w->stream));
      if (err_mask) PVW_HIP(hipMemcpyAsync(err_mask + s0 * words, d_mask, cnt * words * 8, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    }));
    if (col_err) PVW_HIP(hipMemcpyAsync(col_err, d_col, count * 4, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}
}  // extern "C++"

int32_t pvw_shamir_reconstruct_corrected_device(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices,
                                                size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                size_t point_stride, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                uint64_t* d_err_mask, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, d_shares, d_out));
  PVW_TRY(correct_device_checks(r));
  return corrected_device_call(c, r, d_shares, nullptr, d_out, d_nerr, d_col_err, d_err_mask, stream,
                               "corrected reconstruction under stream capture: run a call with the same degree and count and at least as "
                               "many secrets on this stream outside capture first (it sizes the workspace)");
}

int32_t pvw_shamir_reconstruct_corrected(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                         const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                         uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_checks(r, shares, out));
  PVW_TRY(correct_device_checks(r));
  return corrected_host_call(c, r, shares, nullptr, out, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ evaluation of the corrected polynomials
// The decode of 8.11, then values[s][j] = F_s(targets[j] + 1) for every decodable row (0 for the others).  One decode yields
// out, nerr, col_err, err_mask and values.
// device: the bounds of the kernels' 32-bit counts as well; num_targets is bounded BEFORE the targets are read, so a refused count
// costs no walk over the array (the host routine has no such bound and reads every target)
static int32_t evaluate_checks(const Reconstruct<NarrowCalls>& r, const void* shares, const uint64_t* targets, size_t num_targets, const void* values,
                               bool device) {
  PVW_TRY(reconstruct_checks(r, shares, values));            // values stands where the corrected call has out: out may be NULL here
  if (!targets) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (num_targets == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no targets to evaluate at");
  if (device) {
    if (num_targets >= ((size_t)1 << 31)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_targets must be below 2^31 on the device");
    PVW_TRY(correct_device_checks(r));
  }
  for (size_t j = 0; j < num_targets; ++j)
    if (targets[j] >= r.p - 1) return fail(PVW_ERR_INVALID_PARAMETERS, "target index out of range for plain_modulus");
  return PVW_OK;
}

int32_t pvw_shamir_evaluate_corrected_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                           const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                           const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                           uint32_t* col_err, uint64_t* err_mask) {
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_checks(r, shares, targets, num_targets, values, false));
  berlekamp_welch_host(r, shares, out, nerr, col_err, err_mask, targets, num_targets, values);
  return PVW_OK;
}

extern "C++" {
// One pass: ns <= lay.cl.cap secrets from d_shares are decoded (their out, nerr and mask rows; col_err is added to) and evaluated
// at all targets, group by group, into d_values (rows num_targets elements apart).  `resident` is the first target of the group
// whose public matrices the block holds; with one group they are built once for all passes.
template <class F>
static int32_t evaluate_pass_enqueue(pvw_ctx* c, const Reconstruct<F>& r, const typename F::KMod& m, const EvaluateLayout<F>& lay, u64* ws,
                                     const u64* d_shares, size_t ns, size_t secret_stride, size_t point_stride,
                                     const EvalTargets& targets, size_t num_targets, u64* d_values, u64* d_out, u32* d_nerr, u32* d_col_err,
                                     u64* d_mask, size_t* resident, hipStream_t s, const u64* d_erased) {
  constexpr size_t EW = F::EW;
  if (!d_out) d_out = ws + lay.outs;
  if (!d_nerr) d_nerr = (u32*)(ws + lay.nerr);
  PVW_TRY(correct_piece_enqueue(c, r, m, lay.cl, ws, d_shares, ns, secret_stride, point_stride, d_out, d_nerr, d_col_err, d_mask, s, d_erased));
  const u64 *x = ws + lay.cl.pub, *aux = x + r.count * EW;
  const u64 *M = ws, *Lam = ws + lay.cl.lam;
  u64 *YM = ws + lay.ym, *raw = ws + lay.raw, *LamT = ws + lay.lamT, *LamD = ws + lay.lamD, *pub = ws + lay.pub;
  const size_t nk = lay.cl.nk;
  {
    ProfScope ps(c, F::kEvaluate, s);
    PVW_HIP(F::ym(d_shares, secret_stride, point_stride, M, YM, (u32)ns, (u32)r.count, m, s));
  }
  for (size_t j0 = 0; j0 < num_targets; j0 += lay.Tg) {
    const size_t tg = num_targets - j0 < lay.Tg ? num_targets - j0 : lay.Tg;
    if (*resident != j0) {
      ProfScope ps(c, F::kEvaluateWeights, s);
      PVW_HIP(F::target_points(targets, j0, tg, pub, m, s));
      PVW_HIP(F::evaluate_weights(x, aux, pub, r.count, (u32)nk, tg, m, s));
      *resident = j0;
    }
    ProfScope ps(c, F::kEvaluate, s);
    const u64 *scale = pub + tg * EW, *C = scale + tg * EW, *Xt = C + r.count * tg * EW, *Xd = Xt + nk * tg * EW;
    const u32* coin = (const u32*)(Xd + nk * tg * EW);
    typename F::Matmul a{};
    a.A = YM, a.secret_stride = r.count, a.term_stride = 1;
    a.W = C, a.out = raw;
    a.ns = (u32)ns, a.terms = (u32)r.count, a.T = (u32)tg, a.m = m;
    PVW_HIP(F::matmul(a, s));
    typename F::Matmul b{};
    b.A = Lam, b.secret_stride = nk, b.term_stride = 1;
    b.W = Xt, b.out = LamT;
    b.ns = (u32)ns, b.terms = (u32)nk, b.T = (u32)tg, b.m = m;
    PVW_HIP(F::matmul(b, s));
    b.W = Xd, b.out = LamD;
    PVW_HIP(F::matmul(b, s));
    typename F::EvalFinish f{};
    f.shares = d_shares, f.secret_stride = secret_stride, f.point_stride = point_stride;
    f.M = M, f.nerr = d_nerr, f.raw = raw, f.scale = scale, f.coin = coin;
    f.values = d_values + j0 * EW, f.value_stride = num_targets;
    f.ns = (u32)ns, f.count = (u32)r.count, f.Tg = (u32)tg, f.m = m;
    PVW_HIP(F::evaluate_finish(f, LamT, LamD, s));
  }
  return PVW_OK;
}

// The device call of 8.13 or 8.22 behind its argument checks; with d_erased (r.erasures) the decode is that of 8.16 or 8.21
// (corrected_device_call)
template <class F>
static int32_t evaluate_device_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* d_shares, const u64* d_erased, const EvalTargets& targets,
                                    size_t num_targets, u64* d_values, u64* d_out, u32* d_nerr, u32* d_col_err, u64* d_err_mask, void* stream,
                                    const char* unsized) {
  constexpr size_t EW = F::EW;
  const typename F::KMod m = F::kmod(r.p);
  const size_t Tg = evaluate_group(r, num_targets, group_budget());
  const EvaluateLayout<F> lay(r, evaluate_piece(r, Tg, piece_budget()), Tg);
  const size_t need = evaluate_need_bytes(r, Tg, piece_budget());
  if (need < lay.bytes()) return fail(PVW_ERR_INTERNAL, F::kLayoutBound);
  const size_t words = (r.count + 63) / 64;
  // the caller's stream is checked before the context initialises its device (checked_device_call)
  auto sized = [&](hipStream_t s) { return grown_capture_check(c, s, F::correct_bytes, need, unsized); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(correct_block<F>(w, need, {{0, lay.cl.m_bytes()}, {lay.ym, lay.secret_bytes()}}, s));
    u64* ws = w->*F::correct;
    PVW_TRY(correct_weights(c, r, m, lay.cl, ws, s));
    PVW_HIP(launch_shamir_zero_counts(d_col_err, r.count, s));
    size_t resident = SIZE_MAX;
    return correct_passes(r.S, lay.cl.cap, [&](size_t s0, size_t ns) {
      return evaluate_pass_enqueue(c, r, m, lay, ws, d_shares + s0 * r.secret_stride * EW, ns, r.secret_stride, r.point_stride, targets,
                                   num_targets, d_values + s0 * num_targets * EW, Report::from(d_out, s0 * EW), Report::from(d_nerr, s0),
                                   d_col_err, Report::from(d_err_mask, s0 * words), &resident, s, Report::from(d_erased, s0 * words));
    });
  });
}

// host buffers: staged as corrected_host_call stages (each piece one pass over the kernels, the mask rows with their shares); the
// values of a piece come down as one block.  The staged shares, secrets and values, M, y o M and raw are cleared before the call
// returns.
template <class F>
static int32_t evaluate_host_call(pvw_ctx* c, const Reconstruct<F>& r, const u64* shares, const u64* erased, const EvalTargets& targets,
                                  size_t num_targets, u64* values, u64* out, u32* nerr, u32* col_err, u64* err_mask) {
  PVW_TRY(ensure_device(c));
  constexpr size_t EB = F::EW * 8;                               // bytes per element
  const typename F::KMod m = F::kmod(r.p);
  const size_t count = r.count, words = (count + 63) / 64;
  const size_t Tg = evaluate_group(r, num_targets, group_budget());
  size_t per = chunk_1gib((count + 1 + num_targets) * EB + (words + (erased ? words : 0)) * 8 + 4, r.S);
  if (per > evaluate_piece(r, Tg, piece_budget())) per = evaluate_piece(r, Tg, piece_budget());
  const EvaluateLayout<F> lay(r, per, Tg);
  Scratch sc;
  const size_t r_sh = sc.add(per * count * EB), r_out = sc.add(per * EB), r_val = sc.add(per * num_targets * EB), r_ws = sc.add(lay.bytes()),
               r_nerr = sc.add(per * 4), r_col = sc.add(count * 4), r_mask = sc.add(per * words * 8),
               r_er = sc.add(erased ? per * words * 8 : 0);
  ShareStaging<F> st(r, shares, per);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    u64 *d_sh = sc.at(r_sh), *d_out = sc.at(r_out), *d_val = sc.at(r_val), *ws = sc.at(r_ws);
    ws_mark_secret(w, d_sh, (size_t)((char*)ws - (char*)d_sh) + lay.cl.m_bytes());   // staged shares | secrets | values | M
    ws_mark_secret(w, ws + lay.ym, lay.secret_bytes());                              // y o M | raw | the stand-in for out
    u32 *d_nerr = sc.at<u32>(r_nerr), *d_col = col_err ? sc.at<u32>(r_col) : nullptr;
    u64* d_mask = err_mask ? sc.at(r_mask) : nullptr;
    if (erased) st.erased = erased, st.d_erased = sc.at(r_er);
    PVW_TRY(correct_weights(c, r, m, lay.cl, ws, w->stream));
    PVW_HIP(launch_shamir_zero_counts(d_col, count, w->stream));
    size_t resident = SIZE_MAX;
    PVW_TRY(st.run(d_sh, w->stream, [&](size_t s0, size_t cnt) -> int32_t {
      PVW_TRY(evaluate_pass_enqueue(c, r, m, lay, ws, d_sh, cnt, count, 1, targets, num_targets, d_val, d_out, d_nerr, d_col, d_mask, &resident,
                                    w->stream, st.d_erased));
      PVW_HIP(hipMemcpyAsync(values + s0 * num_targets * F::EW, d_val, cnt * num_targets * EB, hipMemcpyDeviceToHost, w->stream));
      if (out) PVW_HIP(hipMemcpyAsync(out + s0 * F::EW, d_out, cnt * EB, hipMemcpyDeviceToHost, w->stream));
      if (nerr) PVW_HIP(hipMemcpyAsync(nerr + s0, d_nerr, cnt * 4, hipMemcpyDeviceToHost, w->stream));
      if (err_mask) PVW_HIP(hipMemcpyAsync(err_mask + s0 * words, d_mask, cnt * words * 8, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    }));
    if (col_err) PVW_HIP(hipMemcpyAsync(col_err, d_col, count * 4, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}
}  // extern "C++"

int32_t pvw_shamir_evaluate_corrected_device(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                             const uint64_t* d_shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                             const uint64_t* targets, size_t num_targets, uint64_t* d_values, uint64_t* d_out,
                                             uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_checks(r, d_shares, targets, num_targets, d_values, true));
  return evaluate_device_call(c, r, d_shares, nullptr, EvalTargets::indices(targets), num_targets, d_values,
                              d_out, d_nerr, d_col_err, d_err_mask, stream,
                              "corrected evaluation under stream capture: run a call with the same degree and count, at least as many "
                              "targets and at least as many secrets on this stream outside capture first (it sizes the workspace)");
}

int32_t pvw_shamir_evaluate_corrected(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                      const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                      const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                      uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_checks(r, shares, targets, num_targets, values, true));
  return evaluate_host_call(c, r, shares, nullptr, EvalTargets::indices(targets), num_targets, values,
                            out, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ reconstruction with erasures
// erased [num_secrets][W], W = ceil(count / 64), in the layout of err_mask: share (s, c) is known to be bad.  With eps_s erased
// columns in row s and E_s = (r - eps_s) / 2, row s is decodable iff eps_s <= r and some F_s of degree <= t disagrees with the row
// in at most E_s of the columns that are not erased: 8.11's definition on the sub-row, which is what the host form runs.
// erased == NULL is the call of 8.11 or 8.13, its bounds included: every entry point hands such a call over as it is.

extern "C++" {
// The contract in plain C++, for both fields: per row the columns that are not erased are compacted, the field's Berlekamp-Welch
// (F::decode: berlekamp_welch_host or berlekamp_welch_wide_host) decodes that sub-row
// with the same t, and the mask bits and col_err go back to the original columns.  A row with fewer than t + 1 columns left
// (eps_s > r) is undecodable.  Nothing at an erased position is read.
template <class F>
static void erasures_host(const Reconstruct<F>& r, const u64* shares, const u64* erased, u64* out, u32* nerr, u32* col_err, u64* err_mask,
                          const u64* targets, size_t num_targets, u64* values) {
  constexpr size_t EW = F::EW;
  const size_t count = r.count, words = (count + 63) / 64;
  std::vector<size_t> cols;
  std::vector<u64> sub_idx(count), sub_sh(count * EW), sub_mask(words);
  std::vector<u32> sub_col(count);
  if (col_err) std::fill(col_err, col_err + count, 0u);
  for (size_t s = 0; s < r.S; ++s) {
    cols.clear();
    for (size_t c = 0; c < count; ++c)
      if (!((erased[s * words + c / 64] >> (c % 64)) & 1)) cols.push_back(c);
    if (err_mask) std::fill(err_mask + s * words, err_mask + (s + 1) * words, (u64)0);
    const size_t n = cols.size();
    if (n < (size_t)r.degree + 1) {
      if (out) std::fill(out + s * EW, out + (s + 1) * EW, (u64)0);
      if (nerr) nerr[s] = PVW_SHAMIR_UNDECODABLE;
      if (values) std::fill(values + s * num_targets * EW, values + (s + 1) * num_targets * EW, (u64)0);
      continue;
    }
    for (size_t i = 0; i < n; ++i) {
      sub_idx[i] = r.indices[cols[i]];
      memcpy(&sub_sh[i * EW], shares + (s * r.secret_stride + cols[i] * r.point_stride) * EW, EW * 8);
    }
    Reconstruct<F> sub = r;                                                        // one dense row of n columns, no mask
    sub.indices = sub_idx.data(), sub.count = n, sub.S = 1, sub.secret_stride = n, sub.point_stride = 1, sub.erasures = false;
    u32 ne = 0;
    F::decode(sub, sub_sh.data(), out ? out + s * EW : nullptr, &ne, sub_col.data(), sub_mask.data(), targets, num_targets,
              values ? values + s * num_targets * EW : nullptr);
    if (nerr) nerr[s] = ne;
    for (size_t i = 0; i < n; ++i)
      if ((sub_mask[i / 64] >> (i % 64)) & 1) {
        if (col_err) ++col_err[cols[i]];
        if (err_mask) err_mask[s * words + cols[i] / 64] |= (u64)1 << (cols[i] % 64);
      }
  }
  volatile u64* vp = sub_sh.data();                                              // as secret as the shares
  for (size_t i = 0; i < sub_sh.size(); ++i) vp[i] = 0;
}
}  // extern "C++"
// on the device the errata locator of a row has up to r + 1 coefficients, in one wave's LDS
static int32_t erasures_device_checks(const Reconstruct<NarrowCalls>& r) {
  if (r.red() + 1 > PVW_SHAMIR_MAX_LOCATOR) {
    char buf[160];
    snprintf(buf, sizeof buf, "on the device the locator of a row with erasures holds at most %d coefficients: count - degree - 1 must be "
             "below %d", PVW_SHAMIR_MAX_LOCATOR, PVW_SHAMIR_MAX_LOCATOR);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  return PVW_OK;
}
static const char* const kErasuresUnsized =
    "reconstruction with erasures under stream capture: run a call with an erasure mask, the same degree and count, at least as many "
    "targets and at least as many secrets on this stream outside capture first (it sizes the workspace)";

int32_t pvw_shamir_reconstruct_erasures_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                             const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                             const uint64_t* erased, uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_reconstruct_corrected_host(plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride, out,
                                                 nerr, col_err, err_mask);
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_checks(r, shares, out));
  erasures_host(r, shares, erased, out, nerr, col_err, err_mask, nullptr, 0, nullptr);
  return PVW_OK;
}
int32_t pvw_shamir_reconstruct_erasures_device(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                               const uint64_t* d_shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                               const uint64_t* d_erased, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                               uint64_t* d_err_mask, void* stream) {
  if (!d_erased)
    return pvw_shamir_reconstruct_corrected_device(c, plain_modulus, degree, indices, count, d_shares, num_secrets, secret_stride,
                                                   point_stride, d_out, d_nerr, d_col_err, d_err_mask, stream);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_checks(r, d_shares, d_out));
  PVW_TRY(correct_device_checks(r));
  PVW_TRY(erasures_device_checks(r));
  return corrected_device_call(c, r, d_shares, d_erased, d_out, d_nerr, d_col_err, d_err_mask, stream, kErasuresUnsized);
}
int32_t pvw_shamir_reconstruct_erasures(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                        const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                        const uint64_t* erased, uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_reconstruct_corrected(c, plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride, out,
                                            nerr, col_err, err_mask);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_checks(r, shares, out));
  PVW_TRY(correct_device_checks(r));
  PVW_TRY(erasures_device_checks(r));
  return corrected_host_call(c, r, shares, erased, out, nerr, col_err, err_mask);
}

int32_t pvw_shamir_evaluate_erasures_host(uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                          const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                          const uint64_t* erased, const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out,
                                          uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_evaluate_corrected_host(plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride, targets,
                                              num_targets, values, out, nerr, col_err, err_mask);
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_checks(r, shares, targets, num_targets, values, false));
  erasures_host(r, shares, erased, out, nerr, col_err, err_mask, targets, num_targets, values);
  return PVW_OK;
}
int32_t pvw_shamir_evaluate_erasures_device(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                            const uint64_t* d_shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                            const uint64_t* d_erased, const uint64_t* targets, size_t num_targets, uint64_t* d_values,
                                            uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask, void* stream) {
  if (!d_erased)
    return pvw_shamir_evaluate_corrected_device(c, plain_modulus, degree, indices, count, d_shares, num_secrets, secret_stride, point_stride,
                                                targets, num_targets, d_values, d_out, d_nerr, d_col_err, d_err_mask, stream);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_checks(r, d_shares, targets, num_targets, d_values, true));
  PVW_TRY(erasures_device_checks(r));
  return evaluate_device_call(c, r, d_shares, d_erased, EvalTargets::indices(targets), num_targets, d_values,
                              d_out, d_nerr, d_col_err, d_err_mask, stream, kErasuresUnsized);
}
int32_t pvw_shamir_evaluate_erasures(pvw_ctx* c, uint64_t plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                     const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                     const uint64_t* erased, const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out,
                                     uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_evaluate_corrected(c, plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride, targets,
                                         num_targets, values, out, nerr, col_err, err_mask);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const Reconstruct<NarrowCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_checks(r, shares, targets, num_targets, values, true));
  PVW_TRY(erasures_device_checks(r));
  return evaluate_host_call(c, r, shares, erased, EvalTargets::indices(targets), num_targets, values,
                            out, nerr, col_err, err_mask);
}

// The mask from a decrypt report: bit (s, c) set iff status(s, c) & status_bits or noise(s, c) > noise_bound; either array may be
// NULL, not both; element (s, c) at s * secret_stride + c * point_stride; every word of mask_out [num_secrets][W] is written.
static int32_t erasure_mask_checks(const void* status, const void* noise, size_t count, size_t num_secrets, size_t secret_stride,
                                   size_t point_stride, const void* mask_out) {
  if ((!status && !noise) || !mask_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares to flag");
  if (num_secrets == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no secrets to reconstruct");
  if (secret_stride == 0 || point_stride == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a stride of 0");
  return PVW_OK;
}
int32_t pvw_shamir_erasure_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound, size_t count,
                                     size_t num_secrets, size_t secret_stride, size_t point_stride, uint64_t* mask_out) {
  PVW_TRY(erasure_mask_checks(status, noise, count, num_secrets, secret_stride, point_stride, mask_out));
  const size_t words = (count + 63) / 64;
  std::fill(mask_out, mask_out + num_secrets * words, (u64)0);
  for (size_t s = 0; s < num_secrets; ++s)
    for (size_t c = 0; c < count; ++c) {
      const size_t off = s * secret_stride + c * point_stride;
      if ((status && (status[off] & status_bits)) || (noise && noise[off] > noise_bound)) mask_out[s * words + c / 64] |= (u64)1 << (c % 64);
    }
  return PVW_OK;
}
int32_t pvw_shamir_erasure_mask_device(pvw_ctx* c, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits,
                                       uint64_t noise_bound, size_t count, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                       uint64_t* d_mask_out, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(erasure_mask_checks(d_status, d_noise, count, num_secrets, secret_stride, point_stride, d_mask_out));
  if (count >= ((size_t)1 << 31) || num_secrets >= ((size_t)1 << 31))
    return fail(PVW_ERR_INVALID_PARAMETERS, "count and num_secrets must be below 2^31 on the device");
  // no scratch of its own; under capture the stream's workspace must exist already, as for the calls the mask is made for
  auto sized = [&](hipStream_t s) {
    return grown_capture_check(c, s, &Workspace::correct_bytes, 0,
                               "erasure mask under stream capture: run a call on this stream outside capture first (it makes the stream's "
                               "workspace)");
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace*, hipStream_t s) -> int32_t {
    ProfScope ps(c, "shamir_erasure_mask", s);
    PVW_HIP(launch_shamir_erasure_mask(d_status, d_noise, status_bits, noise_bound, (u32)count, (u32)num_secrets, secret_stride, point_stride,
                                       d_mask_out, s));
    return PVW_OK;
  });
}

// One call's Shamir sharing on the device (pvw_shamir_shares*, and pvw_deal_shares* through encrypt_multi_enqueue)
struct ShamirDeal {
  const u64* d_secrets;   // [D][words()]
  const u64* d_coeffs;    // [D][degree], or NULL: drawn from the dealers' keys
  u32 degree;
  Mod m;
  u32 pack = 0;           // the packed entry points: secrets per dealer, >= 1, and the packed kernel runs; 0: the calls of 8.9
  const u64* d_packw = nullptr;   // ... on the weights of the call (shamir_packed_prepare)
  const struct ShamirWideDeal* wide = nullptr;   // the wide entry points: the dealers of a pass are these, cut into limbs
  u32 words() const { return pack ? pack : 1; }   // secrets per dealer
  // the same deal starting i dealers further on
  ShamirDeal from(size_t i) const {
    ShamirDeal d = *this;
    d.d_secrets = d_secrets + i * words();
    d.d_coeffs = d_coeffs ? d_coeffs + i * degree : nullptr;
    return d;
  }
};
static size_t shamir_packed_bytes(const pvw_ctx* c, u32 pack) { return shamir_packed_words(pack, c->rowsB()) * 8; }
// Under stream capture a packed call may not allocate: the stream's workspace must hold the weights of at least as many
// pack x columns words already, which an earlier call on that stream outside capture leaves (grown_capture_check)
static int32_t packed_capture_check(pvw_ctx* c, hipStream_t s, u32 pack) {
  return grown_capture_check(c, s, &Workspace::packw_bytes, shamir_packed_bytes(c, pack),
                             "multi-dealer encrypt under stream capture: run a packed call with at least this pack on this stream "
                             "outside capture first (it sizes the weights), and call pvw_prepare(PVW_PREPARE_MFMA)");
}
// once per call: Lw and zt of (p, pack, party range) into the stream's workspace, made on the device (a captured call replays
// without reading host memory); public
static int32_t shamir_packed_prepare(pvw_ctx* c, Workspace* w, ShamirDeal* deal, hipStream_t s) {
  PVW_TRY(ws_grow(&w->packw, &w->packw_bytes, shamir_packed_bytes(c, deal->pack), s, false));
  ProfScope ps(c, "shamir_packed_weights", s);
  PVW_HIP(launch_shamir_packed_weights(w->packw, deal->pack, c->party_lo, c->party_hi, deal->m, s));
  deal->d_packw = w->packw;
  return PVW_OK;
}
// the shares of dealers [0, D) into d_shares [D][n] (columns [party_lo, party_hi)), PVW_MAX_PROLOGUE_KEYS dealers per launch
static int32_t shamir_enqueue(pvw_ctx* c, const ShamirDeal& deal, const DealerKeys& keys, size_t D, u64* d_shares, hipStream_t s) {
  ProfScope ps(c, deal.pack ? "shamir_eval_packed" : "shamir_eval", s);
  for (size_t d0 = 0; d0 < D; d0 += PVW_MAX_PROLOGUE_KEYS) {
    const ShamirDeal dd = deal.from(d0);
    ShamirBatch b{};
    b.nd = (u32)((D - d0) < PVW_MAX_PROLOGUE_KEYS ? (D - d0) : PVW_MAX_PROLOGUE_KEYS);
    b.secrets = dd.d_secrets;
    b.coeffs = dd.d_coeffs;
    b.shares = d_shares + d0 * c->n;
    b.row_stride = c->n;
    b.degree = deal.degree;
    b.party_lo = c->party_lo;
    b.party_hi = c->party_hi;
    b.m = deal.m;
    if (!b.coeffs && deal.degree) keys.from(d0).fill(b, b.nd);
    b.pack = deal.pack;                                        // 0: the unpacked kernel, and the weights are NULL
    b.Lw = deal.d_packw;
    b.zt = deal.d_packw + (size_t)deal.pack * c->rowsB();
    PVW_HIP(launch_shamir_eval(b, s));
    memset(&b, 0, sizeof b);
  }
  return PVW_OK;
}

// One call's sharing over a prime below 2^256.  num_limbs == 0: the shares themselves, [dealer][n][4];
// otherwise vector v = d * num_limbs + w is limb w of dealer d, and key_stride = num_limbs: dealer d draws under vector d * num_limbs's key
struct ShamirWideDeal {
  const u64* d_secrets;   // [D][4]
  const u64* d_coeffs;    // [D][degree][4], or NULL: drawn
  u32 degree;
  WideMod m;
  u32 limb_bits = 0, num_limbs = 0;
  u32 pack = 0;           // the packed entry points: secrets per dealer, d_secrets [D][pack][4], and the packed kernel runs
  const u64* d_packw = nullptr;   // ... on the weights of the call (shamir_packed_wide_prepare)
  WideMont mm{};          // ... with the constants of the general product
};
static size_t shamir_packed_wide_bytes(const pvw_ctx* c, u32 pack) { return shamir_packed_wide_words(pack, c->rowsB()) * 8; }
// packed_capture_check for the wide weights, a block of their own
static int32_t packed_wide_capture_check(pvw_ctx* c, hipStream_t s, u32 pack) {
  return grown_capture_check(c, s, &Workspace::packw_wide_bytes, shamir_packed_wide_bytes(c, pack),
                             "multi-dealer encrypt under stream capture: run a packed wide call with at least this pack on this stream "
                             "outside capture first (it sizes the weights), and call pvw_prepare(PVW_PREPARE_MFMA)");
}
// once per call: Lw and zt of (p, pack, party range) into the stream's workspace, made on the device; public
static int32_t shamir_packed_wide_prepare(pvw_ctx* c, Workspace* w, ShamirWideDeal* deal, hipStream_t s) {
  PVW_TRY(ws_grow(&w->packw_wide, &w->packw_wide_bytes, shamir_packed_wide_bytes(c, deal->pack), s, false));
  ProfScope ps(c, "shamir_packed_wide_weights", s);
  PVW_HIP(launch_shamir_packed_wide_weights(w->packw_wide, deal->pack, c->party_lo, c->party_hi, deal->m, deal->mm, s));
  deal->d_packw = w->packw_wide;
  return PVW_OK;
}
// rows [v0, v0 + nv) of the call (dealers when num_limbs == 0, limb vectors otherwise) into out; `keys` is the source of the
// call's (piece's) vector 0.  PVW_MAX_PROLOGUE_KEYS dealers per launch; a dealer whose limbs straddle two passes is evaluated
// in both and stores only the rows of each (the arithmetic is exact).
static int32_t shamir_wide_enqueue(pvw_ctx* c, const ShamirWideDeal& deal, const DealerKeys& keys, size_t v0, size_t nv, u64* out,
                                   hipStream_t s) {
  if (!nv) return PVW_OK;
  ProfScope ps(c, deal.pack ? "shamir_eval_packed_wide" : "shamir_eval_wide", s);
  const u32 NL = deal.num_limbs, ks = NL ? NL : 1;
  const size_t dlo = v0 / ks, dhi = (v0 + nv - 1) / ks + 1;
  struct OneKey { ChaChaKey key[1]; const RndState* rnd; u64 rnd_off; };
  for (size_t d0 = dlo; d0 < dhi; d0 += PVW_MAX_PROLOGUE_KEYS) {
    ShamirWidePackedBatch pb{};                                   // the unpacked launch takes its first member alone
    ShamirWideBatch& b = pb.b;
    b.secrets = deal.d_secrets;
    b.coeffs = deal.d_coeffs;
    b.row_stride = c->n;
    b.d_lo = (u32)d0;
    b.nd = (u32)((dhi - d0) < PVW_MAX_PROLOGUE_KEYS ? (dhi - d0) : PVW_MAX_PROLOGUE_KEYS);
    b.degree = deal.degree;
    b.party_lo = c->party_lo;
    b.party_hi = c->party_hi;
    b.limb_bits = deal.limb_bits;
    b.num_limbs = NL;
    b.v0 = (u32)v0;
    b.nv = (u32)nv;
    b.out = out;
    b.m = deal.m;
    b.key_stride = ks;
    if (!b.coeffs && deal.degree)
      for (u32 x = 0; x < b.nd; ++x) {
        OneKey k{};
        keys.from((d0 + x) * ks).fill(k, 1);
        b.key[x] = k.key[0];
        if (x == 0) { b.rnd = k.rnd; b.rnd_off = k.rnd_off; }
        memset(&k, 0, sizeof k);
      }
    if (deal.pack) {
      pb.pack = deal.pack;
      pb.Lw = deal.d_packw;
      pb.zt = deal.d_packw + (size_t)deal.pack * c->rowsB() * 4;
      pb.mm = deal.mm;
      PVW_HIP(launch_shamir_eval_packed_wide(pb, s));
    } else {
      PVW_HIP(launch_shamir_eval_wide(b, s));
    }
    memset(&pb, 0, sizeof pb);
  }
  return PVW_OK;
}

// The front of the four calls below: the NULL-argument rule, then the rules of the sharing.
static int32_t shamir_shares_checks(const pvw_ctx* c, const uint64_t* secrets, size_t D, const uint32_t* pack, uint32_t degree, uint64_t p,
                                    const uint8_t* seeds, const uint64_t* coeffs, const uint64_t* shares) {
  if (!c || !secrets || !shares || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  return shamir_checks(c, D, degree, p, pack);
}

// device pointers.  pack != NULL (the packed form): secrets [D][*pack]; the weights once per call, then the packed
// kernel per launch of dealers
static int32_t shamir_shares_device(pvw_ctx* c, const uint64_t* d_secrets, size_t D, const uint32_t* pack, uint32_t degree, uint64_t p,
                                    const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares, void* stream) {
  PVW_TRY(shamir_shares_checks(c, d_secrets, D, pack, degree, p, seeds, d_coeffs, d_shares));
  ShamirDeal deal{d_secrets, d_coeffs, degree, shamir_mod(p), pack ? *pack : 0};
  const DealerKeys keys = DealerKeys::host(seeds);
  if (!pack) {                                                 // no workspace: no device_call
    PVW_TRY(ensure_device(c));
    return shamir_enqueue(c, deal, keys, D, d_shares, call_stream(c, stream));
  }
  // the caller's stream is checked before the context initialises its device (checked_device_call)
  auto sized = [&](hipStream_t s) { return packed_capture_check(c, s, *pack); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(shamir_packed_prepare(c, w, &deal, s));
    return shamir_enqueue(c, deal, keys, D, d_shares, s);
  });
}

// host buffers: the dealers go up in pieces of `per` (secrets [*pack] each, explicit coefficients), each piece's shares come down,
// and the staging -- secrets, coefficients and shares alike -- is cleared when the call ends.  pack != NULL (8.14): the weights once, in front
static int32_t shamir_shares_stage(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, const uint32_t* pack, uint32_t degree,
                                   uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  PVW_TRY(shamir_shares_checks(c, secrets, num_dealers, pack, degree, plain_modulus, seeds, coeffs, shares_out));
  PVW_TRY(ensure_device(c));
  const size_t n = c->n, t = degree, K = pack ? *pack : 1, rB = c->rowsB();
  const size_t per = chunk_1gib((n + (coeffs ? t : 0) + K) * 8, num_dealers);
  Scratch sc;
  const size_t r_se = sc.add(per * K * 8), r_co = sc.add(coeffs ? per * t * 8 : 0), r_sh = sc.add(per * n * 8);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    sc.secret(w, r_se, r_sh);                                  // secrets, coefficients and shares alike
    u64 *d_se = sc.at(r_se), *d_co = coeffs && t ? sc.at(r_co) : nullptr, *d_sh = sc.at(r_sh);
    ShamirDeal deal{d_se, d_co, degree, shamir_mod(plain_modulus), pack ? *pack : 0};
    if (pack) PVW_TRY(shamir_packed_prepare(c, w, &deal, w->stream));
    for (size_t d0 = 0; d0 < num_dealers; d0 += per) {
      const size_t cnt = (num_dealers - d0) < per ? (num_dealers - d0) : per;
      PVW_HIP(hipMemcpyAsync(d_se, secrets + d0 * K, cnt * K * 8, hipMemcpyHostToDevice, w->stream));
      if (d_co) PVW_HIP(hipMemcpyAsync(d_co, coeffs + d0 * t, cnt * t * 8, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(shamir_enqueue(c, deal, DealerKeys::host(seeds).from(d0), cnt, d_sh, w->stream));
      // a sharded context writes its own columns only
      if (rB) PVW_HIP(hipMemcpy2DAsync(shares_out + d0 * n + c->party_lo, n * 8, d_sh + c->party_lo, n * 8, rB * 8, cnt,
                                       hipMemcpyDeviceToHost, w->stream));
      PVW_HIP(hipStreamSynchronize(w->stream));                // the next pass reuses the staging
    }
    return PVW_OK;
  });
}

int32_t pvw_shamir_shares_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                 uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares,
                                 void* stream) {
  return shamir_shares_device(c, d_secrets, num_dealers, nullptr, degree, plain_modulus, seeds, d_coeffs, d_shares, stream);
}
int32_t pvw_shamir_shares(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                          const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  return shamir_shares_stage(c, secrets, num_dealers, nullptr, degree, plain_modulus, seeds, coeffs, shares_out);
}
int32_t pvw_shamir_shares_packed_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                        uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares,
                                        void* stream) {
  return shamir_shares_device(c, d_secrets, num_dealers, &pack, degree, plain_modulus, seeds, d_coeffs, d_shares, stream);
}
int32_t pvw_shamir_shares_packed(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                 uint64_t plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  return shamir_shares_stage(c, secrets, num_dealers, &pack, degree, plain_modulus, seeds, coeffs, shares_out);
}

// ------------------------------------------------------------------------ multi-dealer encrypt
// encrypt_all_party_shares (encryption.rs:253-286): dealer d encrypts scalars[d][0..n) with its own
// randomness (seed d).  Groups of 4 dealers share one pass over A-hat / B-hat (mac_rows_multi).
// Device layout: d_scalars [D][n]; d_c1 [D][rowsA][L][l]; d_c2 [D][rowsB][L][l].
// keys: dealer d's seed, or call_seed(S, c + d) of a device state, with c the counter when the call's kernels run; the
// call's last kernel then advances the counter by D.
// deal != NULL (pvw_deal_shares*): d_scalars is not read; the scalars of each pass of dealers are their Shamir
// shares, made into w->shares by shamir_enqueue in front of the pass (under the same keys, domain DOM_SHAMIR).
static int32_t encrypt_multi_enqueue(pvw_ctx* c, Workspace* w, const u64* d_scalars, const DealerKeys& keys, size_t D, u64* d_c1,
                                     u64* d_c2, uint32_t out_repr, hipStream_t s, const ShamirDeal* deal = nullptr) {
  const u32 k = c->k, l = c->l, L = c->L, rA = c->rowsA(), rB = c->rowsB();
  const size_t P = c->poly();
  const bool use_gemm = multi_uses_gemm(D);
  if (use_gemm) {
    PVW_TRY(ws_gemm_buffers(c, w));
    PVW_TRY(ensure_xm(c, s));
  }
  const size_t group = use_gemm ? (size_t)16 * gemm_vb() : 4;
  // matrix-core passes: the c2 finish pass draws e2 and encodes the scalars itself (tuning build: PVW_FUSED_E2=0 the prologue does)
  const bool fused_e2 = use_gemm && l <= 32 && PVW_ENV_INT("PVW_FUSED_E2", 1) != 0;
  u64* vh = use_gemm ? w->vhat16 : w->rhat;
  if (!use_gemm) ws_public(w, w->rhat, w->rhat_bytes);   // the dealers' r-hat (a deal has marked the block: it stays secret)
  RndState* rs = keys.state();
  for (size_t d0 = 0; d0 < D; d0 += group) {
    const u32 nv = (u32)((D - d0) < group ? (D - d0) : group);
    const u64* gsc = deal ? w->shares : d_scalars + d0 * c->n;   // the pass's scalars [nv][n]
    if (deal && deal->wide) PVW_TRY(shamir_wide_enqueue(c, *deal->wide, keys, d0, nv, w->shares, s));   // vectors [d0, d0 + nv) of the piece
    else if (deal) PVW_TRY(shamir_enqueue(c, deal->from(d0), keys.from(d0), nv, w->shares, s));
    // prologue: the (r, e1, e2) families of dealer d0 replicated over the nv dealers of this pass (up to 64 keys
    // per launch): r-hat_d -> vh[v], NTT(e1), NTT(e2) + m*g-hat -> output planes
    for (u32 v0 = 0; v0 < nv; v0 += PVW_MAX_PROLOGUE_KEYS) {
      const u32 cnt = (nv - v0) < PVW_MAX_PROLOGUE_KEYS ? (nv - v0) : PVW_MAX_PROLOGUE_KEYS;
      const size_t d = d0 + v0;
      PrologueBatch pb{};
      PVW_TRY(fill_encrypt_jobs(c, pb, 0, ExplicitRnd{}, gsc + (size_t)v0 * c->n, vh + (size_t)v0 * k * P,
                                d_c1 + d * rA * P, d_c2 + d * rB * P));
      keys.from(d).fill(pb, cnt);                               // replica x: dealer d + x
      pb.job[0].rep_key = pb.job[1].rep_key = pb.job[2].rep_key = 1;
      pb.job[0].rep_out = (size_t)k * P;                       // r-hat vectors
      pb.job[1].rep_out = (size_t)rA * P;                      // c1 planes
      pb.job[2].rep_out = (size_t)rB * P;                      // c2 planes
      pb.job[2].rep_scalars = c->n;
      pb.njobs = fused_e2 ? 2 : 3;                              // fused: e2 + m g-hat are made by the c2 finish pass
      pb.reps = cnt;
      ProfScope ps(c, "prologue", s);
      PVW_HIP(launch_prologue(pb, c->dt, L, l, s));
    }
    u64* c1g = d_c1 + d0 * rA * P;
    u64* c2g = d_c2 + d0 * rB * P;
    const bool last = d0 + nv == D;                             // its last kernel advances the randomness state
    if (use_gemm) {
      {
        ProfScope ps(c, "vec_digits", s);
        PVW_HIP(launch_vec_digits(vh, (size_t)k * P, w->yd, w->sy, nv, k, L, l, c->dt, s, 0, 0, c->xm_bytes));
      }
      ProfScope ps(c, "gemm_digits", s);
      GemmSection a{c->xmA, c1g, c1g, w->gtmpA, rA, 0, 0}, b{c->xmB, c2g, c2g, w->gtmpB, rB, 0, 0};
      std::vector<GemmErrSource> es;
      if (fused_e2) {
        // e2_d[i] (encryption.rs:195-196): dealer d's key, stream DOM_E2 / party index, uniform in [-b2, b2]; + m_{d,i} g-hat
        for (u32 v0 = 0; v0 < nv; v0 += PVW_MAX_PROLOGUE_KEYS) {
          GemmErrSource e{};
          e.span = (nv - v0) < PVW_MAX_PROLOGUE_KEYS ? (nv - v0) : PVW_MAX_PROLOGUE_KEYS;
          keys.from(d0 + v0).fill(e, e.span);                  // vector x: dealer d0 + v0 + x
          e.key_v = 1;
          e.domain = DOM_E2; e.index0 = c->party_lo; e.index_row = 1; e.index_v = 0; e.bound = c->b2;
          e.scalars = gsc + c->party_lo; e.scalar_v = c->n;
          es.push_back(e);
        }
        b.addend = nullptr;
      }
      if (rs && last) {
        GemmSection& fin = rB ? b : a;                          // the finish pass launched last
        fin.rnd_ctr = &rs->counter;
        fin.rnd_adv = D;
      }
      PVW_HIP(launch_gemm_digits(a, b, w->yd, w->sy, c->dt, k, L, l, nv, (size_t)rA * P, (size_t)rB * P, s, nullptr, fused_e2 ? es.data() : nullptr, c->xm_bytes));
    } else {
      ProfScope ps(c, "mac_rows_multi", s);
      MacSection a(c->dA, c1g, c1g, rA), b(c->dB, c2g, c2g, rB);
      MultiVec mv{vh, (size_t)k * P, (size_t)rA * P, (size_t)rB * P, nv};
      if (rs && last) {
        a.rnd_ctr = &rs->counter;
        a.rnd_adv = D;
      }
      PVW_HIP(launch_mac_rows_multi(a, b, mv, c->dt, k, L, l, s));
    }
  }
  if (out_repr == PVW_REPR_POWER) {
    ProfScope ps(c, "intt", s);
    PVW_HIP(launch_ntt(d_c1, D * rA, true, c->dt, L, l, s));
    PVW_HIP(launch_ntt(d_c2, D * rB, true, c->dt, L, l, s));
  }
  return PVW_OK;
}

static int32_t encrypt_multi_checks(pvw_ctx* c, size_t D, size_t per_dealer, uint32_t out_repr) {
  PVW_TRY(check_repr(out_repr));
  if (D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no dealers");
  if (per_dealer != c->n) {                                                          // encryption.rs:264-274
    char buf[96];
    snprintf(buf, sizeof buf, "Dealer provided %zu shares but needs %u", per_dealer, c->n);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (c->num_keys < c->party_hi)
    return fail(PVW_ERR_INVALID_PARAMETERS, "Global public key is not complete (missing party keys)");
  if (!c->crs_loaded) return fail(PVW_ERR_CRS, "CRS not loaded");
  int32_t ok = 0;
  pvw_ctx_verify_correctness_condition(c, &ok);
  if (!ok) return fail(PVW_ERR_INVALID_PARAMETERS, "Parameters do not satisfy correctness condition - decryption may fail");
  return PVW_OK;
}

// what a deal leaves in the workspace: the shares, and below the matrix-core threshold the dealers' r-hat in the vectors the
// workspace shares with key material (with r-hat a share is c2 - <b-hat, r-hat>; pvw_selftest_secret_residue always scans them)
static void deal_mark(Workspace* w, size_t D) {
  ws_mark_secret(w, w->shares, w->shares_bytes);
  if (!multi_uses_gemm(D)) ws_mark_secret(w, w->rhat, w->rhat_bytes);
}

// host buffers, staged in pieces of `per` dealers (<= ~512 MiB of ciphertext): each dealer's input -- its n scalars, or with
// deal != NULL its `pack` secrets -- goes up, the piece is encrypted, and its rows go to their global positions
static int32_t encrypt_multi_stage(pvw_ctx* c, const uint64_t* in, size_t D, const DealerKeys& keys, const ShamirDeal* deal,
                                   uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  const size_t P = c->poly(), rA = c->rowsA(), rB = c->rowsB(), n = c->n, in_words = deal ? deal->words() : n;
  size_t per = stage_budget() / 2 / ((rA + rB) * P * 8 + in_words * 8);
  if (per < 4) per = 4;
  per &= ~(size_t)3;
  if (per > D) per = D;
  Scratch sc;
  const size_t r_in = sc.add(per * in_words * 8), r_c1 = sc.add(per * rA * P * 8), r_c2 = sc.add(per * rB * P * 8);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    if (deal) {
      PVW_TRY(ws_share_buffer(c, w));
      sc.secret(w, r_in, r_in);
      deal_mark(w, per);                                           // each pass takes the matrix cores or the VALU by its OWN dealer
      if (D % per) deal_mark(w, D % per);                          // count: a last pass of 1 or 2 leaves r-hat in the workspace
    }
    u64 *d_in = sc.at(r_in), *d_c1 = sc.at(r_c1), *d_c2 = sc.at(r_c2);
    ShamirDeal staged = deal ? *deal : ShamirDeal{};                // the secrets of each piece
    staged.d_secrets = d_in;
    if (deal && deal->pack) PVW_TRY(shamir_packed_prepare(c, w, &staged, w->stream));
    for (size_t d0 = 0; d0 < D; d0 += per) {
      const size_t cnt = (D - d0) < per ? (D - d0) : per;
      PVW_HIP(hipMemcpyAsync(d_in, in + d0 * in_words, cnt * in_words * 8, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(encrypt_multi_enqueue(c, w, deal ? nullptr : d_in, keys.piece(d0), cnt, d_c1, d_c2, out_repr, w->stream, deal ? &staged : nullptr));
      for (size_t d = 0; d < cnt; ++d) {
        // a sharded context writes its rows at their global positions inside each dealer's block
        PVW_HIP(hipMemcpyAsync(c1_out + ((d0 + d) * c->k + c->c1_lo) * P, d_c1 + d * rA * P, rA * P * 8, hipMemcpyDeviceToHost, w->stream));
        PVW_HIP(hipMemcpyAsync(c2_out + ((d0 + d) * n + c->party_lo) * P, d_c2 + d * rB * P, rB * P * 8, hipMemcpyDeviceToHost, w->stream));
      }
      if (deal && d0 + cnt < D) PVW_HIP(hipStreamSynchronize(w->stream));   // the next piece reuses the pageable staging
    }
    return PVW_OK;
  });
}

// The four multi-dealer frames, in the order of encrypt's; their seed and _rs exports differ in the key source alone.
static int32_t encrypt_multi_device(pvw_ctx* c, const uint64_t* d_scalars, size_t D, size_t per_dealer, const DealerKeys& keys,
                                    uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  if (!c || !d_scalars || keys.missing() || (!d_c1 && c->rowsA()) || (!d_c2 && c->rowsB())) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_multi_checks(c, D, per_dealer, out_repr));
  return device_call(c, stream, [&](hipStream_t s) -> int32_t {
                       PVW_TRY(keys.checks(c));
                       return multi_capture_check(c, s, D);
                     },
                     [&](Workspace* w, hipStream_t s) { return encrypt_multi_enqueue(c, w, d_scalars, keys, D, d_c1, d_c2, out_repr, s); });
}
static int32_t encrypt_multi_host(pvw_ctx* c, const uint64_t* scalars, size_t D, size_t per_dealer, const DealerKeys& keys,
                                  uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  if (!c || !scalars || keys.missing() || !c1_out || !c2_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_multi_checks(c, D, per_dealer, out_repr));
  PVW_TRY(ensure_device(c));
  PVW_TRY(keys.checks(c));
  return encrypt_multi_stage(c, scalars, D, keys, nullptr, c1_out, c2_out, out_repr);
}
// the deal on device pointers: encrypt_multi_enqueue with the shares made pass by pass in the workspace's share scratch, which
// the call marks secret (cleared on the stream behind the call's last launch)
// pack != NULL (pvw_deal_shares_packed*): secrets [D][*pack], the weights once per call and the packed kernel, whatever
// *pack; under capture the caller's stream is checked before the context initialises its device, as pvw_shamir_shares_packed_device does
static int32_t deal_device(pvw_ctx* c, const uint64_t* d_secrets, size_t D, uint32_t degree, uint64_t p, const DealerKeys& keys,
                           uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream, const uint32_t* pack = nullptr) {
  if (!c || !d_secrets || keys.missing() || (!d_c1 && c->rowsA()) || (!d_c2 && c->rowsB())) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_multi_checks(c, D, c->n, out_repr));
  PVW_TRY(shamir_checks(c, D, degree, p, pack));
  ShamirDeal deal{d_secrets, nullptr, degree, shamir_mod(p), pack ? *pack : 0};
  if (pack && stream) PVW_TRY(packed_capture_check(c, (hipStream_t)stream, *pack));
  return device_call(c, stream, [&](hipStream_t s) -> int32_t {
                       PVW_TRY(keys.checks(c));
                       if (pack) PVW_TRY(packed_capture_check(c, s, *pack));
                       return deal_capture_check(c, s, D);
                     },
                     [&](Workspace* w, hipStream_t s) -> int32_t {
                       PVW_TRY(ws_share_buffer(c, w));
                       deal_mark(w, D);
                       if (pack) PVW_TRY(shamir_packed_prepare(c, w, &deal, s));
                       return encrypt_multi_enqueue(c, w, nullptr, keys, D, d_c1, d_c2, out_repr, s, &deal);
                     });
}
static int32_t deal_host(pvw_ctx* c, const uint64_t* secrets, size_t D, uint32_t degree, uint64_t p, const DealerKeys& keys,
                         uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr, const uint32_t* pack = nullptr) {
  if (!c || !secrets || keys.missing() || !c1_out || !c2_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_multi_checks(c, D, c->n, out_repr));
  PVW_TRY(shamir_checks(c, D, degree, p, pack));
  PVW_TRY(ensure_device(c));
  PVW_TRY(keys.checks(c));
  // the staging loop points it at each piece's secrets in turn, and makes the weights of a packed deal
  const ShamirDeal deal{nullptr, nullptr, degree, shamir_mod(p), pack ? *pack : 0};
  return encrypt_multi_stage(c, secrets, D, keys, &deal, c1_out, c2_out, out_repr);
}

int32_t pvw_encrypt_multi_device(pvw_ctx* c, const uint64_t* d_scalars, size_t num_dealers, size_t scalars_per_dealer,
                                 const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return encrypt_multi_device(c, d_scalars, num_dealers, scalars_per_dealer, DealerKeys::host(seeds), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_encrypt_multi_rs_device(pvw_ctx* c, const uint64_t* d_scalars, size_t num_dealers, size_t scalars_per_dealer,
                                    void* handle, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return encrypt_multi_device(c, d_scalars, num_dealers, scalars_per_dealer, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_encrypt_multi(pvw_ctx* c, const uint64_t* scalars, size_t num_dealers, size_t scalars_per_dealer,
                          const uint8_t* seeds, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return encrypt_multi_host(c, scalars, num_dealers, scalars_per_dealer, DealerKeys::host(seeds), c1_out, c2_out, out_repr);
}
int32_t pvw_encrypt_multi_rs(pvw_ctx* c, const uint64_t* scalars, size_t num_dealers, size_t scalars_per_dealer,
                             void* handle, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return encrypt_multi_host(c, scalars, num_dealers, scalars_per_dealer, DealerKeys::state(handle), c1_out, c2_out, out_repr);
}
int32_t pvw_deal_shares_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                               const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return deal_device(c, d_secrets, num_dealers, degree, plain_modulus, DealerKeys::host(seeds), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_deal_shares_rs_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                                  void* handle, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return deal_device(c, d_secrets, num_dealers, degree, plain_modulus, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_deal_shares(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                        const uint8_t* seeds, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_host(c, secrets, num_dealers, degree, plain_modulus, DealerKeys::host(seeds), c1_out, c2_out, out_repr);
}
int32_t pvw_deal_shares_rs(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, uint64_t plain_modulus,
                           void* handle, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_host(c, secrets, num_dealers, degree, plain_modulus, DealerKeys::state(handle), c1_out, c2_out, out_repr);
}

int32_t pvw_deal_shares_packed_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                      uint64_t plain_modulus, const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr,
                                      void* stream) {
  return deal_device(c, d_secrets, num_dealers, degree, plain_modulus, DealerKeys::host(seeds), d_c1, d_c2, out_repr, stream, &pack);
}
int32_t pvw_deal_shares_packed_rs_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                         uint64_t plain_modulus, void* handle, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr,
                                         void* stream) {
  return deal_device(c, d_secrets, num_dealers, degree, plain_modulus, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream, &pack);
}
int32_t pvw_deal_shares_packed(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                               uint64_t plain_modulus, const uint8_t* seeds, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_host(c, secrets, num_dealers, degree, plain_modulus, DealerKeys::host(seeds), c1_out, c2_out, out_repr, &pack);
}
int32_t pvw_deal_shares_packed_rs(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                  uint64_t plain_modulus, void* handle, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_host(c, secrets, num_dealers, degree, plain_modulus, DealerKeys::state(handle), c1_out, c2_out, out_repr, &pack);
}

// ------------------------------------------------------------------------ Shamir shares over a prime below 2^256
// Elements of four words; the host side runs the kernel's own arithmetic (pvw_wide.h), scaled as the kernel runs it.
typedef u64 Wide[4];
static void wide_set(Wide o, const u64* a) { for (int i = 0; i < 4; ++i) o[i] = a[i]; }
static void wide_small(Wide o, u64 v) { o[0] = v; o[1] = o[2] = o[3] = 0; }
static bool wide_is_zero(const Wide a) { return !(a[0] | a[1] | a[2] | a[3]); }
// a, b below pn: (a + b) mod pn and (a - b) mod pn
static void wide_addmod(Wide a, const Wide b, const WideMod& m) {
  u64 r[4];
  wide_set(r, a);
  wide_step(r, 1, *(const u64(*)[4])b, m);
  wide_set(a, r);
}
static void wide_negmod(Wide a, const WideMod& m) {   // pn - a, 0 stays 0
  if (wide_is_zero(a)) return;
  u64 br = 0;
  for (int i = 0; i < 4; ++i) {
    const u64 s1 = m.pn[i] - a[i], s2 = s1 - br;
    br = (m.pn[i] < a[i]) | (s1 < br);
    a[i] = s2;
  }
}
// res = a b mod p, scaled: a scaled and below pn, b ANY four words (its 16-bit digits are the multipliers of 32 steps)
static void wide_mulmod(Wide res, const Wide a, const Wide b, const WideMod& m) {
  u64 r[4] = {0, 0, 0, 0}, zero[4] = {0, 0, 0, 0}, av[4];
  wide_set(av, a);
  for (int k = 16; k-- > 0;) {
    const u32 dg = (u32)(b[k / 4] >> (16 * (k % 4))) & 0xFFFF;
    wide_step(r, 1u << 16, zero, m);
    u64 t[4];
    wide_set(t, av);
    wide_step(t, dg, r, m);
    wide_set(r, t);
  }
  wide_set(res, r);
}
// a scaled -> the plain words of a, and back
static void wide_unscale(Wide o, const Wide a, const WideMod& m) {
  u64 t[4];
  wide_set(t, a);
  wide_shr(t, m.shift);
  wide_set(o, t);
}
static void wide_reduce(Wide o, const u64* w, const WideMod& m) {
  u64 t[4];
  wide_reduce_scaled(w, m, t);
  wide_set(o, t);
}
// a^e mod p (scaled in, scaled out), e any four words
static void wide_powmod(Wide res, const Wide a, const Wide e, const WideMod& m) {
  Wide r, one, b, plain;
  wide_small(one, 1);
  wide_reduce(r, one, m);
  wide_set(b, a);
  for (int i = 255; i >= 0; --i) {
    wide_unscale(plain, r, m);
    wide_mulmod(r, r, plain, m);
    if ((e[i / 64] >> (i % 64)) & 1) {
      wide_unscale(plain, b, m);
      wide_mulmod(r, r, plain, m);
    }
  }
  wide_set(res, r);
}
static void wide_invmod(Wide res, const Wide a, const Wide p, const WideMod& m) {   // Fermat: a^(p - 2)
  Wide e;
  wide_set(e, p);
  u64 br = 2;
  for (int i = 0; i < 4 && br; ++i) {
    const u64 v = e[i];
    e[i] = v - br;
    br = v < br;
  }
  wide_powmod(res, a, e, m);
}

// Miller-Rabin over the first 32 primes as bases (include/pvw_hip.h states the list); p odd and >= 3
static const u32 WIDE_MR_BASES[32] = {2,  3,  5,  7,  11, 13, 17, 19, 23, 29, 31, 37,  41,  43,  47,  53,
                                      59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131};
static bool wide_is_prime(const Wide p, const WideMod& m) {
  if (!p[1] && !p[2] && !p[3]) return is_prime_u64(p[0]);
  Wide pm1, dd, one, onep, m1;
  wide_set(pm1, p);
  pm1[0] -= 1;                                             // p odd
  wide_set(dd, pm1);
  u32 r = 0;
  while (!(dd[0] & 1)) {
    u64 t[4];
    wide_set(t, dd);
    wide_shr(t, 1);
    wide_set(dd, t);
    ++r;
  }
  wide_small(one, 1);
  wide_reduce(onep, one, m);
  wide_reduce(m1, pm1, m);
  for (u32 bi = 0; bi < 32; ++bi) {
    Wide a, x;
    wide_small(a, WIDE_MR_BASES[bi]);
    wide_reduce(a, a, m);
    wide_powmod(x, a, dd, m);
    if (!memcmp(x, onep, 32) || !memcmp(x, m1, 32)) continue;
    bool witness = true;
    for (u32 i = 1; i < r && witness; ++i) {
      Wide plain;
      wide_unscale(plain, x, m);
      wide_mulmod(x, x, plain, m);
      if (!memcmp(x, m1, 32)) witness = false;
    }
    if (witness) return false;
  }
  return true;
}

// p odd, >= 3 and prime; the verdict of the last modulus a thread asked about is kept (a protocol runs many calls on one field)
static int32_t wide_modulus_check(const uint64_t* p, WideMod* out) {
  if (!p) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!(p[0] & 1) || (p[0] < 3 && !p[1] && !p[2] && !p[3]))
    return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be an odd prime (Shamir shares live in a field)");
  *out = make_wide_mod(p);
  static thread_local u64 known[4] = {0, 0, 0, 0};
  if (memcmp(known, p, 32) != 0) {
    if (!wide_is_prime(p, *out)) return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be prime (Shamir shares live in a field)");
    memcpy(known, p, 32);
  }
  return PVW_OK;
}
static int32_t wide_limb_count(const WideMod& m, uint32_t limb_bits, uint32_t* num_limbs) {
  if (limb_bits < 16 || limb_bits > 62) return fail(PVW_ERR_INVALID_PARAMETERS, "limb_bits must be in [16, 62]");
  const u32 nl = (m.bits + limb_bits - 1) / limb_bits;
  if (nl > PVW_WIDE_MAX_LIMBS) return fail(PVW_ERR_INVALID_PARAMETERS, "more than 16 limbs: choose wider limbs");
  *num_limbs = nl;
  return PVW_OK;
}
// The rules of both wide dealing families.  pack != NULL: the rules of 8.18 first, then the packed ones.
static int32_t shamir_wide_checks(const pvw_ctx* c, size_t D, uint32_t degree, const uint64_t* p, WideMod* m, const uint32_t* pack = nullptr) {
  if (D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no dealers");
  if (!p) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!p[1] && !p[2] && !p[3] && p[0] <= c->n)
    return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must exceed the party count (evaluation points 1..n)");
  PVW_TRY(wide_modulus_check(p, m));
  if (degree >= c->n) {
    char buf[112];
    snprintf(buf, sizeof buf, "degree %u needs more than %u parties", degree, c->n);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (!pack) return PVW_OK;
  const u64 K = *pack, n = c->n;
  if (K == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at least 1");
  if (K > PVW_WIDE_MAX_PACK) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at most PVW_WIDE_MAX_PACK");
  if ((u64)degree + K > n) {
    char buf[128];
    snprintf(buf, sizeof buf, "degree %u with pack %u needs at least %llu parties", degree, *pack, (unsigned long long)degree + K);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (n + K - 1 >= ((u64)1 << 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "n + pack - 1 must be below 2^32");
  if (!p[1] && !p[2] && !p[3] && p[0] < n + K)
    return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be at least n + pack (the points 1..n and 0, -1, .., -(pack-1) are distinct)");
  return PVW_OK;
}

int32_t pvw_shamir_wide_limbs(const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t* num_limbs) {
  if (!plain_modulus || !num_limbs) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!(plain_modulus[0] & 1) || (plain_modulus[0] < 3 && !plain_modulus[1] && !plain_modulus[2] && !plain_modulus[3]))
    return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be an odd prime (Shamir shares live in a field)");
  return wide_limb_count(make_wide_mod(plain_modulus), limb_bits, num_limbs);
}

// the contract on the host cores (no GPU), through the kernel's own step.  Writes all n columns, whatever the context's shard.
int32_t pvw_shamir_shares_wide_host(const pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree,
                                    const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  if (!c || !secrets || !shares_out || !plain_modulus || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(shamir_wide_checks(c, num_dealers, degree, plain_modulus, &m));
  const u32 n = c->n, t = degree;
  std::vector<u64> a(((size_t)t + 1) * 4);
  for (size_t d = 0; d < num_dealers; ++d) {
    wide_reduce(&a[0], secrets + d * 4, m);
    for (u32 j = 1; j <= t; ++j) {
      if (coeffs) wide_reduce(&a[(size_t)j * 4], coeffs + (d * t + (j - 1)) * 4, m);
      else wide_draw_scaled(make_key(seeds + d * 32), PVW_DOM_SHAMIR, j, m, *(u64(*)[4]) & a[(size_t)j * 4]);
    }
    for (u32 i = 0; i < n; ++i) {
      u64 acc[4] = {0, 0, 0, 0};
      for (u32 e = t + 1; e-- > 0;) wide_step(acc, i + 1, *(const u64(*)[4]) & a[(size_t)e * 4], m);
      wide_shr(acc, m.shift);
      wide_set(shares_out + (d * n + i) * 4, acc);
    }
  }
  volatile u64* va = a.data();                               // the coefficients are as secret as the secret
  for (size_t j = 0; j < a.size(); ++j) va[j] = 0;
  return PVW_OK;
}

// the packed contract on the host cores, by the definition: the weights L_j(i + 1) and Z(i + 1) once per call (one
// inversion, of (K-1)!), then per share t steps and K + 1 products.  Writes all n columns.
int32_t pvw_shamir_shares_packed_wide_host(const pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                           const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs,
                                           uint64_t* shares_out) {
  if (!c || !secrets || !shares_out || !plain_modulus || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(shamir_wide_checks(c, num_dealers, degree, plain_modulus, &m, &pack));
  const u32 n = c->n, t = degree, K = pack;
  const u64 zero[4] = {0, 0, 0, 0};
  Wide one, ones, f, inv, fj, plain;
  wide_small(one, 1);
  wide_reduce(ones, one, m);                                 // 1, scaled
  // w_j = (-1)^j / (j! (K-1-j)!), plain
  std::vector<u64> invf((size_t)K * 4), wj((size_t)K * 4);
  wide_set(f, ones);
  for (u32 j = 2; j < K; ++j) {
    wide_small(fj, j);
    wide_mulmod(f, f, fj, m);
  }
  wide_invmod(inv, f, plain_modulus, m);
  for (u32 j = K - 1;; --j) {
    wide_set(&invf[(size_t)j * 4], inv);                     // 1 / j!, scaled
    if (j == 0) break;
    wide_small(fj, j);
    wide_mulmod(inv, inv, fj, m);
  }
  for (u32 j = 0; j < K; ++j) {
    Wide v;
    wide_unscale(plain, &invf[(size_t)(K - 1 - j) * 4], m);
    wide_mulmod(v, &invf[(size_t)j * 4], plain, m);
    if (j & 1) wide_negmod(v, m);
    wide_unscale(&wj[(size_t)j * 4], v, m);
  }
  // Lw[j][i] = L_j(i + 1) and zt[i] = Z(i + 1), plain
  std::vector<u64> Lw((size_t)K * n * 4), zt((size_t)n * 4), sufv((size_t)K * 4);
  for (u32 i = 0; i < n; ++i) {
    u64 suf[4], pre[4];
    wide_set(suf, ones);
    for (u32 j = K; j-- > 0;) {
      wide_set(&sufv[(size_t)j * 4], suf);
      wide_step(suf, i + 1 + j, zero, m);                    // i + K < 2^32
    }
    wide_unscale(&zt[(size_t)i * 4], suf, m);
    wide_set(pre, ones);
    for (u32 j = 0; j < K; ++j) {
      Wide v;
      wide_unscale(plain, pre, m);
      wide_mulmod(v, &sufv[(size_t)j * 4], plain, m);
      wide_mulmod(v, v, &wj[(size_t)j * 4], m);
      wide_unscale(&Lw[((size_t)j * n + i) * 4], v, m);
      wide_step(pre, i + 1 + j, zero, m);
    }
  }
  std::vector<u64> a(((size_t)t + 1) * 4), sec((size_t)K * 4);
  for (size_t d = 0; d < num_dealers; ++d) {
    for (u32 j = 0; j < K; ++j) wide_reduce(&sec[(size_t)j * 4], secrets + (d * K + j) * 4, m);
    for (u32 j = 1; j <= t; ++j) {
      if (coeffs) wide_reduce(&a[(size_t)j * 4], coeffs + (d * t + (j - 1)) * 4, m);
      else wide_draw_scaled(make_key(seeds + d * 32), PVW_DOM_SHAMIR, j, m, *(u64(*)[4]) & a[(size_t)j * 4]);
    }
    for (u32 i = 0; i < n; ++i) {
      u64 r[4] = {0, 0, 0, 0};
      for (u32 e = t; e >= 1; --e) wide_step(r, i + 1, *(const u64(*)[4]) & a[(size_t)e * 4], m);   // a_1 + a_2 x + ... + a_t x^(t-1)
      Wide acc, prod;
      wide_mulmod(acc, r, &zt[(size_t)i * 4], m);
      for (u32 j = 0; j < K; ++j) {
        wide_mulmod(prod, &sec[(size_t)j * 4], &Lw[((size_t)j * n + i) * 4], m);
        wide_addmod(acc, prod, m);
      }
      wide_unscale(shares_out + (d * n + i) * 4, acc, m);
    }
  }
  volatile u64* va = a.data();                               // the coefficients are as secret as the secrets
  for (size_t j = 0; j < a.size(); ++j) va[j] = 0;
  volatile u64* vs = sec.data();
  for (size_t j = 0; j < sec.size(); ++j) vs[j] = 0;
  return PVW_OK;
}

int32_t pvw_shamir_wide_to_limbs_host(const uint64_t* values, size_t count, uint32_t limb_bits, uint32_t num_limbs, uint64_t* limbs_out) {
  if ((!values || !limbs_out) && count) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (limb_bits < 16 || limb_bits > 62) return fail(PVW_ERR_INVALID_PARAMETERS, "limb_bits must be in [16, 62]");
  if (num_limbs < 1 || num_limbs > PVW_WIDE_MAX_LIMBS) return fail(PVW_ERR_INVALID_PARAMETERS, "num_limbs must be in [1, 16]");
  const u64 mask = ((u64)1 << limb_bits) - 1;
  for (size_t i = 0; i < count; ++i) {
    u64 v[4];
    wide_set(v, values + i * 4);
    for (u32 w = 0; w < num_limbs; ++w) {
      limbs_out[(size_t)w * count + i] = v[0] & mask;
      wide_shr(v, limb_bits);
    }
    if ((size_t)num_limbs * limb_bits < 256 && !wide_is_zero(v)) return fail(PVW_ERR_INVALID_PARAMETERS, "a value does not fit num_limbs limbs");
  }
  return PVW_OK;
}

int32_t pvw_shamir_wide_from_limbs_host(const uint64_t* plain_modulus, const uint64_t* limbs, size_t count, uint32_t limb_bits,
                                        uint32_t num_limbs, uint64_t* out) {
  if (!plain_modulus || ((!limbs || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (limb_bits < 16 || limb_bits > 62) return fail(PVW_ERR_INVALID_PARAMETERS, "limb_bits must be in [16, 62]");
  if (num_limbs < 1 || num_limbs > PVW_WIDE_MAX_LIMBS) return fail(PVW_ERR_INVALID_PARAMETERS, "num_limbs must be in [1, 16]");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  const u32 h0 = limb_bits / 2, h1 = limb_bits - h0;       // 2^limb_bits in two multipliers below 2^32
  for (size_t i = 0; i < count; ++i) {
    u64 acc[4] = {0, 0, 0, 0}, zero[4] = {0, 0, 0, 0};
    for (u32 w = num_limbs; w-- > 0;) {
      Wide lw;
      wide_small(lw, limbs[(size_t)w * count + i]);
      u64 add[4];
      wide_reduce_scaled(lw, m, add);
      wide_step(acc, 1u << h0, zero, m);
      wide_step(acc, 1u << h1, add, m);
    }
    wide_shr(acc, m.shift);
    wide_set(out + i * 4, acc);
  }
  return PVW_OK;
}

// Lagrange at 0 from the points indices[i] + 1: w_i = prod_{j != i} x_j / (x_j - x_i), one inversion per weight
int32_t pvw_shamir_reconstruct_wide(const uint64_t* plain_modulus, const uint64_t* indices, const uint64_t* shares, size_t count,
                                    size_t num_secrets, uint64_t* out) {
  if (!plain_modulus || !indices || ((!shares || !out) && num_secrets)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  const bool small_p = !plain_modulus[1] && !plain_modulus[2] && !plain_modulus[3];
  {
    std::vector<u64> sorted(indices, indices + count);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < count; ++i) {
      if (i && sorted[i] == sorted[i - 1]) return fail(PVW_ERR_INVALID_PARAMETERS, "duplicate party index");
      if (sorted[i] == ~(u64)0 || (small_p && sorted[i] >= plain_modulus[0] - 1))
        return fail(PVW_ERR_INVALID_PARAMETERS, "party index must be below plain_modulus - 1");
    }
  }
  std::vector<u64> wts(count * 4);
  for (size_t i = 0; i < count; ++i) {
    Wide num, den, one, f;
    wide_small(one, 1);
    wide_reduce(num, one, m);
    wide_set(den, num);
    bool neg = false;
    for (size_t j = 0; j < count; ++j) {
      if (j == i) continue;
      const u64 xj = indices[j] + 1, xi = indices[i] + 1;
      wide_small(f, xj);
      wide_mulmod(num, num, f, m);
      wide_small(f, xj > xi ? xj - xi : xi - xj);
      if (xj < xi) neg = !neg;
      wide_mulmod(den, den, f, m);
    }
    Wide inv, plain;
    wide_invmod(inv, den, plain_modulus, m);
    wide_unscale(plain, inv, m);
    wide_mulmod(num, num, plain, m);
    if (neg) wide_negmod(num, m);
    wide_unscale(&wts[i * 4], num, m);                     // the weight, plain and below p
  }
  for (size_t s = 0; s < num_secrets; ++s) {
    Wide acc, y, prod;
    wide_small(acc, 0);
    for (size_t i = 0; i < count; ++i) {
      wide_reduce(y, shares + (s * count + i) * 4, m);
      wide_mulmod(prod, y, &wts[i * 4], m);
      wide_addmod(acc, prod, m);
    }
    wide_unscale(out + s * 4, acc, m);
  }
  volatile u64* vw = wts.data();
  for (size_t j = 0; j < wts.size(); ++j) vw[j] = 0;
  return PVW_OK;
}

// Lagrange at 0, -1, .., -(pack-1) from the points x_i = indices[i] + 1: the weight of point i at -k is
// prod_{j != i}(x_j + k) / (x_j - x_i).  The denominators do not depend on k: one inversion per point; the numerators of one k
// come from prefix and suffix products of the x_j + k.  Then pack dot products per row.
int32_t pvw_shamir_reconstruct_packed_wide(const uint64_t* plain_modulus, uint32_t pack, const uint64_t* indices, const uint64_t* shares,
                                           size_t count, size_t num_rows, uint64_t* out) {
  if (!plain_modulus || !indices || ((!shares || !out) && num_rows)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no shares");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  if (pack == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at least 1");
  const bool small_p = !plain_modulus[1] && !plain_modulus[2] && !plain_modulus[3];
  {
    u64 pw[4];
    wide_set(pw, plain_modulus);
    std::vector<u64> sorted(indices, indices + count);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < count; ++i) {
      if (i && sorted[i] == sorted[i - 1]) return fail(PVW_ERR_INVALID_PARAMETERS, "duplicate party index");
      if (sorted[i] == ~(u64)0 || (small_p && sorted[i] >= plain_modulus[0] - 1))
        return fail(PVW_ERR_INVALID_PARAMETERS, "party index must be below plain_modulus - 1");
      u64 top[4] = {sorted[i] + pack, 0, 0, 0};            // index + pack as a wide integer
      top[1] = top[0] < sorted[i];
      if (!wide_less(top, pw)) return fail(PVW_ERR_INVALID_PARAMETERS, "party index must be below plain_modulus - pack");
    }
  }
  Wide one, ones;
  wide_small(one, 1);
  wide_reduce(ones, one, m);
  // 1 / prod_{j != i}(x_j - x_i), scaled
  std::vector<u64> dinv(count * 4);
  for (size_t i = 0; i < count; ++i) {
    Wide den, f;
    wide_set(den, ones);
    bool neg = false;
    for (size_t j = 0; j < count; ++j) {
      if (j == i) continue;
      const u64 xj = indices[j] + 1, xi = indices[i] + 1;
      wide_small(f, xj > xi ? xj - xi : xi - xj);
      if (xj < xi) neg = !neg;
      wide_mulmod(den, den, f, m);
    }
    wide_invmod(&dinv[i * 4], den, plain_modulus, m);
    if (neg) wide_negmod(&dinv[i * 4], m);
  }
  // wts[k][i], plain and below p
  std::vector<u64> wts((size_t)pack * count * 4), sufv(count * 4);
  for (u32 k = 0; k < pack; ++k) {
    auto factor = [&](size_t j, Wide f) {                  // x_j + k, at most 2^64 + pack - 2
      const u64 xj = indices[j] + 1;
      f[0] = xj + k;
      f[1] = f[0] < xj;
      f[2] = f[3] = 0;
    };
    Wide suf, pre, f, plain, v;
    wide_set(suf, ones);
    for (size_t j = count; j-- > 0;) {
      wide_set(&sufv[j * 4], suf);
      factor(j, f);
      wide_mulmod(suf, suf, f, m);
    }
    wide_set(pre, ones);
    for (size_t i = 0; i < count; ++i) {
      wide_unscale(plain, pre, m);
      wide_mulmod(v, &sufv[i * 4], plain, m);
      wide_unscale(plain, &dinv[i * 4], m);
      wide_mulmod(v, v, plain, m);
      wide_unscale(&wts[((size_t)k * count + i) * 4], v, m);
      factor(i, f);
      wide_mulmod(pre, pre, f, m);
    }
  }
  for (size_t s = 0; s < num_rows; ++s) {
    std::vector<u64> y(count * 4);
    for (size_t i = 0; i < count; ++i) wide_reduce(&y[i * 4], shares + (s * count + i) * 4, m);
    for (u32 k = 0; k < pack; ++k) {
      Wide acc, prod;
      wide_small(acc, 0);
      for (size_t i = 0; i < count; ++i) {
        wide_mulmod(prod, &y[i * 4], &wts[((size_t)k * count + i) * 4], m);
        wide_addmod(acc, prod, m);
      }
      wide_unscale(out + (s * pack + k) * 4, acc, m);
    }
    volatile u64* vy = y.data();
    for (size_t j = 0; j < y.size(); ++j) vy[j] = 0;
  }
  return PVW_OK;
}

// the front of the device-side shares calls.  pack != NULL: the packed forms
static int32_t shamir_wide_shares_checks(const pvw_ctx* c, const uint64_t* secrets, size_t D, uint32_t degree, const uint64_t* p,
                                         const uint8_t* seeds, const uint64_t* coeffs, const uint64_t* shares, WideMod* m,
                                         const uint32_t* pack = nullptr) {
  if (!c || !secrets || !shares || !p || (degree && !seeds && !coeffs)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  return shamir_wide_checks(c, D, degree, p, m, pack);
}

// device pointers (seeds and plain_modulus stay HOST pointers): no workspace, nothing allocated, may be captured.
// pack != NULL (the packed form): secrets [D][*pack][4]; the weights once per call into the stream's workspace, then
// the packed kernel per launch of dealers
static int32_t shamir_wide_shares_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, const uint32_t* pack, uint32_t degree,
                                         const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares,
                                         void* stream) {
  WideMod m;
  PVW_TRY(shamir_wide_shares_checks(c, d_secrets, num_dealers, degree, plain_modulus, seeds, d_coeffs, d_shares, &m, pack));
  ShamirWideDeal deal{d_secrets, degree ? d_coeffs : nullptr, degree, m};
  const DealerKeys keys = DealerKeys::host(seeds);
  if (!pack) {
    PVW_TRY(ensure_device(c));
    return shamir_wide_enqueue(c, deal, keys, 0, num_dealers, d_shares, call_stream(c, stream));
  }
  deal.pack = *pack;
  deal.mm = make_wide_mont(plain_modulus);
  // the caller's stream is checked before the context initialises its device (checked_device_call)
  auto sized = [&](hipStream_t s) { return packed_wide_capture_check(c, s, *pack); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(shamir_packed_wide_prepare(c, w, &deal, s));
    return shamir_wide_enqueue(c, deal, keys, 0, num_dealers, d_shares, s);
  });
}

// host buffers: the dealers go up in bounded pieces (secrets [*pack][4] each), each piece's shares come down, and the staging is
// cleared when the call ends.  pack != NULL: the weights once, in front
static int32_t shamir_wide_shares_stage(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, const uint32_t* pack, uint32_t degree,
                                        const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  WideMod m;
  PVW_TRY(shamir_wide_shares_checks(c, secrets, num_dealers, degree, plain_modulus, seeds, coeffs, shares_out, &m, pack));
  PVW_TRY(ensure_device(c));
  const size_t n = c->n, t = degree, K = pack ? *pack : 1, rB = c->rowsB();
  const size_t per = chunk_1gib((n + (coeffs ? t : 0) + K) * 32, num_dealers);
  Scratch sc;
  const size_t r_se = sc.add(per * K * 32), r_co = sc.add(coeffs ? per * t * 32 : 0), r_sh = sc.add(per * n * 32);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    sc.secret(w, r_se, r_sh);
    u64 *d_se = sc.at(r_se), *d_co = coeffs && t ? sc.at(r_co) : nullptr, *d_sh = sc.at(r_sh);
    ShamirWideDeal deal{d_se, d_co, degree, m};
    if (pack) {
      deal.pack = *pack;
      deal.mm = make_wide_mont(plain_modulus);
      PVW_TRY(shamir_packed_wide_prepare(c, w, &deal, w->stream));
    }
    for (size_t d0 = 0; d0 < num_dealers; d0 += per) {
      const size_t cnt = (num_dealers - d0) < per ? (num_dealers - d0) : per;
      PVW_HIP(hipMemcpyAsync(d_se, secrets + d0 * K * 4, cnt * K * 32, hipMemcpyHostToDevice, w->stream));
      if (d_co) PVW_HIP(hipMemcpyAsync(d_co, coeffs + d0 * t * 4, cnt * t * 32, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(shamir_wide_enqueue(c, deal, DealerKeys::host(seeds).from(d0), 0, cnt, d_sh, w->stream));
      // a sharded context writes its own columns only
      if (rB) PVW_HIP(hipMemcpy2DAsync(shares_out + (d0 * n + c->party_lo) * 4, n * 32, d_sh + (size_t)c->party_lo * 4, n * 32, rB * 32, cnt,
                                       hipMemcpyDeviceToHost, w->stream));
      PVW_HIP(hipStreamSynchronize(w->stream));                // the next piece reuses the staging
    }
    return PVW_OK;
  });
}

int32_t pvw_shamir_shares_wide_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                      const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs, uint64_t* d_shares,
                                      void* stream) {
  return shamir_wide_shares_device(c, d_secrets, num_dealers, nullptr, degree, plain_modulus, seeds, d_coeffs, d_shares, stream);
}
int32_t pvw_shamir_shares_wide(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, const uint64_t* plain_modulus,
                               const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  return shamir_wide_shares_stage(c, secrets, num_dealers, nullptr, degree, plain_modulus, seeds, coeffs, shares_out);
}
int32_t pvw_shamir_shares_packed_wide_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                             const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* d_coeffs,
                                             uint64_t* d_shares, void* stream) {
  return shamir_wide_shares_device(c, d_secrets, num_dealers, &pack, degree, plain_modulus, seeds, d_coeffs, d_shares, stream);
}
int32_t pvw_shamir_shares_packed_wide(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                      const uint64_t* plain_modulus, const uint8_t* seeds, const uint64_t* coeffs, uint64_t* shares_out) {
  return shamir_wide_shares_stage(c, secrets, num_dealers, &pack, degree, plain_modulus, seeds, coeffs, shares_out);
}

// The deal: pvw_encrypt_multi* on D * NL vectors whose scalars are the limb planes, made pass by pass in the share scratch.
static int32_t deal_wide_front(pvw_ctx* c, const uint64_t* secrets, size_t D, uint32_t degree, const uint64_t* p, uint32_t limb_bits,
                               const DealerKeys& keys, const uint64_t* c1, const uint64_t* c2, bool device, uint32_t out_repr,
                               ShamirWideDeal* deal, const uint32_t* pack) {
  if (!c || !secrets || !p || keys.missing() || (device ? (!c1 && c->rowsA()) || (!c2 && c->rowsB()) : !c1 || !c2))
    return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(encrypt_multi_checks(c, D, c->n, out_repr));
  WideMod m;
  PVW_TRY(shamir_wide_checks(c, D, degree, p, &m, pack));
  u32 nl = 0;
  PVW_TRY(wide_limb_count(m, limb_bits, &nl));
  *deal = ShamirWideDeal{secrets, nullptr, degree, m, limb_bits, nl};
  if (pack) {
    deal->pack = *pack;
    deal->mm = make_wide_mont(p);
  }
  return PVW_OK;
}
// pack != NULL (pvw_deal_shares_packed_wide*): secrets [D][*pack][4], the weights once per call and the packed kernel,
// whatever *pack; under capture the caller's stream is checked before the context initialises its device
static int32_t deal_wide_device(pvw_ctx* c, const uint64_t* d_secrets, size_t D, uint32_t degree, const uint64_t* p, uint32_t limb_bits,
                                const DealerKeys& keys, uint64_t* d_c1, uint64_t* d_c2, uint32_t out_repr, void* stream,
                                const uint32_t* pack = nullptr) {
  ShamirWideDeal wd;
  PVW_TRY(deal_wide_front(c, d_secrets, D, degree, p, limb_bits, keys, d_c1, d_c2, true, out_repr, &wd, pack));
  ShamirDeal deal{nullptr, nullptr, degree, Mod{}, 0};
  deal.wide = &wd;
  const size_t V = D * wd.num_limbs;
  if (pack && stream) PVW_TRY(packed_wide_capture_check(c, (hipStream_t)stream, *pack));
  return device_call(c, stream, [&](hipStream_t s) -> int32_t {
                       PVW_TRY(keys.checks(c));
                       if (pack) PVW_TRY(packed_wide_capture_check(c, s, *pack));
                       return deal_capture_check(c, s, V);
                     },
                     [&](Workspace* w, hipStream_t s) -> int32_t {
                       PVW_TRY(ws_share_buffer(c, w));
                       deal_mark(w, V);
                       if (pack) PVW_TRY(shamir_packed_wide_prepare(c, w, &wd, s));
                       return encrypt_multi_enqueue(c, w, nullptr, keys, V, d_c1, d_c2, out_repr, s, &deal);
                     });
}
// host buffers, staged in pieces of whole dealers (<= ~512 MiB of ciphertext), so that every piece starts on a dealer's first
// vector and its keys are the piece's own
static int32_t deal_wide_host(pvw_ctx* c, const uint64_t* secrets, size_t D, uint32_t degree, const uint64_t* p, uint32_t limb_bits,
                              const DealerKeys& keys, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr,
                              const uint32_t* pack = nullptr) {
  ShamirWideDeal wd;
  PVW_TRY(deal_wide_front(c, secrets, D, degree, p, limb_bits, keys, c1_out, c2_out, false, out_repr, &wd, pack));
  PVW_TRY(ensure_device(c));
  PVW_TRY(keys.checks(c));
  const size_t P = c->poly(), rA = c->rowsA(), rB = c->rowsB(), n = c->n, NL = wd.num_limbs, K = pack ? *pack : 1;   // K * 4 words a dealer
  size_t per = stage_budget() / 2 / (NL * (rA + rB) * P * 8 + K * 32);
  if (per < 1) per = 1;
  if (per > D) per = D;
  Scratch sc;
  const size_t r_in = sc.add(per * K * 32), r_c1 = sc.add(per * NL * rA * P * 8), r_c2 = sc.add(per * NL * rB * P * 8);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_TRY(ws_share_buffer(c, w));
    sc.secret(w, r_in, r_in);
    deal_mark(w, per * NL);
    if (D % per) deal_mark(w, (D % per) * NL);
    u64 *d_in = sc.at(r_in), *d_c1 = sc.at(r_c1), *d_c2 = sc.at(r_c2);
    wd.d_secrets = d_in;
    ShamirDeal deal{nullptr, nullptr, degree, Mod{}, 0};
    deal.wide = &wd;
    if (pack) PVW_TRY(shamir_packed_wide_prepare(c, w, &wd, w->stream));
    for (size_t d0 = 0; d0 < D; d0 += per) {
      const size_t cnt = (D - d0) < per ? (D - d0) : per, nvec = cnt * NL;
      PVW_HIP(hipMemcpyAsync(d_in, secrets + d0 * K * 4, cnt * K * 32, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(encrypt_multi_enqueue(c, w, nullptr, keys.piece(d0 * NL), nvec, d_c1, d_c2, out_repr, w->stream, &deal));
      for (size_t v = 0; v < nvec; ++v) {
        // a sharded context writes its rows at their global positions inside each vector's block
        PVW_HIP(hipMemcpyAsync(c1_out + ((d0 * NL + v) * c->k + c->c1_lo) * P, d_c1 + v * rA * P, rA * P * 8, hipMemcpyDeviceToHost, w->stream));
        PVW_HIP(hipMemcpyAsync(c2_out + ((d0 * NL + v) * n + c->party_lo) * P, d_c2 + v * rB * P, rB * P * 8, hipMemcpyDeviceToHost, w->stream));
      }
      if (d0 + cnt < D) PVW_HIP(hipStreamSynchronize(w->stream));   // the next piece reuses the pageable staging
    }
    return PVW_OK;
  });
}

int32_t pvw_deal_shares_wide(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, const uint64_t* plain_modulus,
                             uint32_t limb_bits, const uint8_t* seeds, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_wide_host(c, secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::host(seeds), c1_out, c2_out, out_repr);
}
int32_t pvw_deal_shares_wide_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                    const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* d_c1, uint64_t* d_c2,
                                    uint32_t out_repr, void* stream) {
  return deal_wide_device(c, d_secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::host(seeds), d_c1, d_c2, out_repr, stream);
}
int32_t pvw_deal_shares_wide_rs(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t degree, const uint64_t* plain_modulus,
                                uint32_t limb_bits, void* handle, uint64_t* c1_out, uint64_t* c2_out, uint32_t out_repr) {
  return deal_wide_host(c, secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::state(handle), c1_out, c2_out, out_repr);
}
int32_t pvw_deal_shares_wide_rs_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t degree,
                                       const uint64_t* plain_modulus, uint32_t limb_bits, void* handle, uint64_t* d_c1, uint64_t* d_c2,
                                       uint32_t out_repr, void* stream) {
  return deal_wide_device(c, d_secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream);
}

int32_t pvw_deal_shares_packed_wide(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                    const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* c1_out,
                                    uint64_t* c2_out, uint32_t out_repr) {
  return deal_wide_host(c, secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::host(seeds), c1_out, c2_out, out_repr, &pack);
}
int32_t pvw_deal_shares_packed_wide_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                           const uint64_t* plain_modulus, uint32_t limb_bits, const uint8_t* seeds, uint64_t* d_c1,
                                           uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return deal_wide_device(c, d_secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::host(seeds), d_c1, d_c2, out_repr, stream,
                          &pack);
}
int32_t pvw_deal_shares_packed_wide_rs(pvw_ctx* c, const uint64_t* secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                       const uint64_t* plain_modulus, uint32_t limb_bits, void* handle, uint64_t* c1_out, uint64_t* c2_out,
                                       uint32_t out_repr) {
  return deal_wide_host(c, secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::state(handle), c1_out, c2_out, out_repr, &pack);
}
int32_t pvw_deal_shares_packed_wide_rs_device(pvw_ctx* c, const uint64_t* d_secrets, size_t num_dealers, uint32_t pack, uint32_t degree,
                                              const uint64_t* plain_modulus, uint32_t limb_bits, void* handle, uint64_t* d_c1,
                                              uint64_t* d_c2, uint32_t out_repr, void* stream) {
  return deal_wide_device(c, d_secrets, num_dealers, degree, plain_modulus, limb_bits, DealerKeys::state(handle), d_c1, d_c2, out_repr, stream,
                          &pack);
}

// SELF-TEST: the kernel's Horner step on the device, out = (acc x + add) mod p
int32_t pvw_selftest_shamir_wide_step(pvw_ctx* c, const uint64_t* plain_modulus, const uint64_t* acc, const uint64_t* x, const uint64_t* add,
                                      size_t count, uint64_t* out) {
  if (!c || !plain_modulus || ((!acc || !x || !add || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  for (size_t i = 0; i < count; ++i) {
    u64 a[4], b[4], pp[4];
    wide_set(a, acc + i * 4);
    wide_set(b, add + i * 4);
    wide_set(pp, plain_modulus);
    if (x[i] >> 32 || !wide_less(a, pp) || !wide_less(b, pp))
      return fail(PVW_ERR_INVALID_PARAMETERS, "the step takes acc, add below plain_modulus and x below 2^32");
  }
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, count * 104));
    u64* base = (u64*)w->scratch;
    u64 *d_acc = base, *d_add = base + count * 4, *d_out = base + count * 8, *d_x = base + count * 12;
    PVW_HIP(hipMemcpyAsync(d_acc, acc, count * 32, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(hipMemcpyAsync(d_add, add, count * 32, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(hipMemcpyAsync(d_x, x, count * 8, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(launch_shamir_wide_step(m, d_acc, d_x, d_add, count, d_out, w->stream));
    PVW_HIP(hipMemcpyAsync(out, d_out, count * 32, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}

// ------------------------------------------------------------------------ the receiving end over a prime below 2^256
// The fold of decrypted limbs on the device, and checked reconstruction with wide elements: the contract of 8.10.

static int32_t wide_fold_checks(const uint64_t* p, const void* limbs, const void* out, size_t count, uint32_t limb_bits, uint32_t num_limbs,
                                WideMod* m) {
  if (!p || ((!limbs || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (limb_bits < 16 || limb_bits > 62) return fail(PVW_ERR_INVALID_PARAMETERS, "limb_bits must be in [16, 62]");
  if (num_limbs < 1 || num_limbs > PVW_WIDE_MAX_LIMBS) return fail(PVW_ERR_INVALID_PARAMETERS, "num_limbs must be in [1, 16]");
  return wide_modulus_check(p, m);
}

// device pointers (plain_modulus stays a HOST pointer): no workspace, nothing allocated, may be captured
int32_t pvw_shamir_wide_from_limbs_device(pvw_ctx* c, const uint64_t* plain_modulus, const uint64_t* d_limbs, size_t count,
                                          size_t limb_stride, size_t elem_stride, uint32_t limb_bits, uint32_t num_limbs, uint64_t* d_out,
                                          void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(wide_fold_checks(plain_modulus, d_limbs, d_out, count, limb_bits, num_limbs, &m));
  if (limb_stride == 0 || elem_stride == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a stride of 0");
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const hipStream_t s = call_stream(c, stream);
  ProfScope ps(c, "shamir_wide_fold", s);
  PVW_HIP(launch_shamir_wide_fold(m, d_limbs, count, limb_stride, elem_stride, limb_bits, num_limbs, d_out, s));
  return PVW_OK;
}

// the order of reconstruct_checks: NULL, no secrets, too few shares, a duplicate, the range, the modulus (which sets r.m), the strides
static int32_t reconstruct_wide_checks(Reconstruct<WideCalls>& r, const void* shares, const void* out) {
  PVW_TRY(reconstruct_front_checks(r, r.p && r.indices && shares && out));
  {
    std::vector<u64> sorted(r.indices, r.indices + r.count);
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < r.count; ++i)
      if (sorted[i] == sorted[i - 1]) return fail(PVW_ERR_INVALID_PARAMETERS, "duplicate party index");
  }
  const bool one_word = !r.p[1] && !r.p[2] && !r.p[3];
  if (one_word && r.p[0] < 2) return fail(PVW_ERR_INVALID_PARAMETERS, "plain_modulus must be prime (Shamir shares live in a field)");
  // the point x = index + 1 <= 2^64 must be below p: p of one word bounds the index; 2^64 itself needs p > 2^64
  const bool above_2_64 = r.p[2] || r.p[3] || r.p[1] > 1 || (r.p[1] == 1 && r.p[0] != 0);
  for (size_t i = 0; i < r.count; ++i)
    if (one_word ? r.indices[i] >= r.p[0] - 1 : (r.indices[i] == ~(u64)0 && !above_2_64))
      return fail(PVW_ERR_INVALID_PARAMETERS, "party index out of range for plain_modulus");
  PVW_TRY(wide_modulus_check(r.p, &r.m));
  if (r.secret_stride == 0 || r.point_stride == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a stride of 0");
  return PVW_OK;
}
// a <- (a - b) mod pn and res = a b mod p for scaled a, b below pn
static void wide_submod(Wide a, const Wide b, const WideMod& m) {
  Wide nb;
  wide_set(nb, b);
  wide_negmod(nb, m);
  wide_addmod(a, nb, m);
}
static void wide_mulmod_scaled(Wide res, const Wide a, const Wide b, const WideMod& m) {
  Wide plain;
  wide_unscale(plain, b, m);
  wide_mulmod(res, a, plain, m);
}

// The contract in plain C++ (no GPU), apart from the kernels in method and in arithmetic: the scaled step of pvw_wide.h, not
// the Montgomery product; for every target the basis polynomials L_j(x) = prod_{i != j}(x - x_i) / prod_{i != j}(x_j - x_i)
// from prefix and suffix products of the factors (x - x_i), then one dot product per secret.
int32_t pvw_shamir_reconstruct_wide_checked_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                 const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                 uint64_t* out, uint32_t* bad, uint32_t* col_bad) {
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  const WideMod& m = r.m;
  const size_t t = degree, T = r.T();
  std::vector<u64> x(count * 4), inv_den((t + 1) * 4), L((t + 1) * 4), suf((t + 2) * 4), basis((t + 1) * 4);
  Wide one;
  {
    Wide w1;
    wide_small(w1, 1);
    wide_reduce(one, w1, m);
  }
  for (size_t c = 0; c < count; ++c) {
    const u64 xw[4] = {indices[c] + 1, indices[c] + 1 == 0 ? (u64)1 : (u64)0, 0, 0};
    wide_reduce(&x[c * 4], xw, m);
  }
  for (size_t j = 0; j <= t; ++j) {
    Wide den, d;
    wide_set(den, one);
    for (size_t i = 0; i <= t; ++i)
      if (i != j) {
        wide_set(d, &x[j * 4]);
        wide_submod(d, &x[i * 4], m);
        wide_mulmod_scaled(den, den, d, m);
      }
    wide_invmod(&inv_den[j * 4], den, plain_modulus, m);
  }
  if (bad) std::fill(bad, bad + num_secrets, 0u);
  if (col_bad) std::fill(col_bad, col_bad + count, 0u);
  for (size_t tm = 0; tm < T; ++tm) {
    Wide xm, d, pre;
    wide_small(xm, 0);
    if (tm) wide_set(xm, &x[(t + tm) * 4]);
    wide_set(&suf[(t + 1) * 4], one);                          // suf[i] = prod_{k >= i, k <= t}(x_m - x_k)
    for (size_t i = t + 1; i-- > 0;) {
      wide_set(d, xm);
      wide_submod(d, &x[i * 4], m);
      wide_mulmod_scaled(&suf[i * 4], &suf[(i + 1) * 4], d, m);
    }
    wide_set(pre, one);                                        // prod_{k < j}(x_m - x_k)
    for (size_t j = 0; j <= t; ++j) {
      Wide v;
      wide_mulmod_scaled(v, pre, &suf[(j + 1) * 4], m);
      wide_mulmod_scaled(&L[j * 4], v, &inv_den[j * 4], m);
      wide_set(d, xm);
      wide_submod(d, &x[j * 4], m);
      wide_mulmod_scaled(pre, pre, d, m);
    }
    for (size_t s = 0; s < num_secrets; ++s) {
      const u64* row = shares + s * secret_stride * 4;
      Wide v, y, prod;
      wide_small(v, 0);
      for (size_t j = 0; j <= t; ++j) {
        wide_reduce(y, row + j * point_stride * 4, m);
        wide_mulmod_scaled(prod, y, &L[j * 4], m);
        wide_addmod(v, prod, m);
      }
      if (tm == 0) {
        wide_unscale(out + s * 4, v, m);
      } else {
        wide_reduce(y, row + (t + tm) * point_stride * 4, m);
        if (memcmp(y, v, 32) != 0) {
          if (bad) ++bad[s];
          if (col_bad) ++col_bad[t + tm];
        }
      }
    }
  }
  return PVW_OK;
}

int32_t pvw_shamir_reconstruct_wide_checked_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                   size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                   size_t point_stride, uint64_t* d_out, uint32_t* d_bad, uint32_t* d_col_bad,
                                                   void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, d_shares, d_out));
  PVW_TRY(reconstruct_device_checks(r));
  return checked_device_call(c, r, d_shares, d_out, d_bad, d_col_bad, stream);
}
// host buffers: staged and run as pvw_shamir_reconstruct_checked is (checked_host_call), in dense [piece][count][4] blocks
int32_t pvw_shamir_reconstruct_wide_checked(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                            const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                            uint64_t* out, uint32_t* bad, uint32_t* col_bad) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  PVW_TRY(reconstruct_device_checks(r));
  return checked_host_call(c, r, shares, out, bad, col_bad);
}

// ------------------------------------------------------------------------ corrected reconstruction below 2^256
// The contract of 8.11 with wide elements: row s is decodable iff some F_s of degree <= t disagrees with it in at most
// E = (count - t - 1) / 2 columns; F_s is then unique, out[s] = F_s(0) and the disagreeing columns are reported.

static inline u64 (&wel(std::vector<u64>& v, size_t i))[4] { return *(u64(*)[4]) & v[i * 4]; }

// The contract in plain C++ (no GPU), by another method than the kernels' (syndromes, Berlekamp-Massey, locator roots):
// Berlekamp-Welch as berlekamp_welch_host runs it, over the Montgomery product of pvw_wide.h with every element times R (a zero
// test and an equality test do not depend on the form; the secret is taken out of it at the end).  Its last step is the
// contract itself: N / W is compared with the row in every column.  Cubic in count per secret.
// With targets, which are FIELD ELEMENTS here, [num_targets][4] plain words below p (the index forms convert targets + 1 into
// them: wide_index_points): values[s][j] = F_s(targets[j]), four plain words, by Horner over the quotient's
// coefficients, 0 for an undecodable row (pvw_shamir_evaluate_wide_corrected_host); out may then be NULL.
static void berlekamp_welch_wide_host(const Reconstruct<WideCalls>& r, const uint64_t* shares, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                      uint64_t* err_mask, const uint64_t* targets = nullptr, size_t num_targets = 0,
                                      uint64_t* values = nullptr) {
  const WideMont mm = make_wide_mont(r.p);
  const size_t count = r.count, t = r.degree, E = (count - t - 1) / 2, nq = t + E + 1, nu = nq + E, ld = nu + 1;
  const size_t words = (count + 63) / 64;
  std::vector<u64> x(count * 4), y(count * 4), A(count * ld * 4), sol(nu * 4), W((E + 1) * 4), N(nq * 4);
  std::vector<size_t> pivot_col;
  const u64 zero[4] = {0, 0, 0, 0};
  auto set = [](u64(&o)[4], const u64(&a)[4]) { for (int i = 0; i < 4; ++i) o[i] = a[i]; };
  auto is0 = [](const u64(&a)[4]) { return !(a[0] | a[1] | a[2] | a[3]); };
  for (size_t c = 0; c < count; ++c) {
    const u64 xw[4] = {r.indices[c] + 1, r.indices[c] + 1 == 0 ? (u64)1 : (u64)0, 0, 0};
    wide_mont_in(xw, mm, wel(x, c));
  }
  if (col_err) std::fill(col_err, col_err + count, 0u);
  for (size_t s = 0; s < r.S; ++s) {
    for (size_t c = 0; c < count; ++c) {
      const u64* sp = shares + (s * r.secret_stride + c * r.point_stride) * 4;
      const u64 w[4] = {sp[0], sp[1], sp[2], sp[3]};
      wide_mont_in(w, mm, wel(y, c));
    }
    // row c: sum_j N_j x^j - y sum_{k < E} W_k x^k = y x^E
    for (size_t c = 0; c < count; ++c) {
      u64 pw[4], v[4];
      set(pw, mm.one);
      for (size_t j = 0; j < nq; ++j) {
        set(wel(A, c * ld + j), pw);
        if (j <= E) {
          wide_mont_mul(wel(y, c), pw, mm, v);
          if (j == E) set(wel(A, c * ld + nu), v);
          else {
            u64 neg[4] = {0, 0, 0, 0};
            wide_sub_p(neg, v, mm);
            set(wel(A, c * ld + nq + j), neg);
          }
        }
        wide_mont_mul(pw, wel(x, c), mm, pw);
      }
    }
    pivot_col.clear();
    size_t rank = 0;
    for (size_t col = 0; col < nu && rank < count; ++col) {
      size_t pr = rank;
      while (pr < count && is0(wel(A, pr * ld + col))) ++pr;
      if (pr == count) continue;
      if (pr != rank) std::swap_ranges(&A[pr * ld * 4], &A[(pr + 1) * ld * 4], &A[rank * ld * 4]);
      u64 inv[4];
      wide_mont_inv(wel(A, rank * ld + col), mm, inv);
      for (size_t j = col; j <= nu; ++j) wide_mont_mul(wel(A, rank * ld + j), inv, mm, wel(A, rank * ld + j));
      for (size_t i = 0; i < count; ++i) {
        u64 f[4];
        set(f, wel(A, i * ld + col));
        if (i == rank || is0(f)) continue;
        for (size_t j = col; j <= nu; ++j) {
          u64 v[4];
          wide_mont_mul(f, wel(A, rank * ld + j), mm, v);
          wide_sub_p(wel(A, i * ld + j), v, mm);
        }
      }
      pivot_col.push_back(col);
      ++rank;
    }
    bool ok = true;
    for (size_t i = rank; i < count && ok; ++i) ok = is0(wel(A, i * ld + nu));   // a row 0 = b: no solution
    u64 secret[4] = {0, 0, 0, 0};
    std::vector<size_t> wrong;
    if (ok) {
      std::fill(sol.begin(), sol.end(), (u64)0);                                 // free unknowns: 0
      for (size_t i = 0; i < rank; ++i) set(wel(sol, pivot_col[i]), wel(A, i * ld + nu));
      for (size_t j = 0; j < nq; ++j) set(wel(N, j), wel(sol, j));
      for (size_t k = 0; k < E; ++k) set(wel(W, k), wel(sol, nq + k));
      set(wel(W, E), mm.one);
      // N / W by long division (W monic): the quotient stays in N[E ..], the remainder in N[.. E)
      for (size_t i = nq; i-- > E;) {
        u64 f[4];
        set(f, wel(N, i));
        for (size_t k = 0; k < E; ++k) {
          u64 v[4];
          wide_mont_mul(f, wel(W, k), mm, v);
          wide_sub_p(wel(N, i - E + k), v, mm);
        }
      }
      for (size_t k = 0; k < E && ok; ++k) ok = is0(wel(N, k));
      if (ok) {
        for (size_t c = 0; c < count; ++c) {                                     // F = N[E ..], degree <= t
          u64 v[4];
          set(v, wel(N, E + t));
          for (size_t j = t; j-- > 0;) {
            wide_mont_mul(v, wel(x, c), mm, v);
            wide_add_p(v, wel(N, E + j), mm);
          }
          if (memcmp(v, &y[c * 4], 32) != 0) wrong.push_back(c);
        }
        ok = wrong.size() <= E;
        wide_mont_out(wel(N, E), mm, secret);
      }
    }
    for (size_t j = 0; j < num_targets; ++j) {
      u64 v[4] = {0, 0, 0, 0};
      if (ok) {
        const u64 xw[4] = {targets[j * 4], targets[j * 4 + 1], targets[j * 4 + 2], targets[j * 4 + 3]};
        u64 xs[4];
        wide_mont_in(xw, mm, xs);
        set(v, wel(N, E + t));
        for (size_t k = t; k-- > 0;) {
          wide_mont_mul(v, xs, mm, v);
          wide_add_p(v, wel(N, E + k), mm);
        }
        wide_mont_out(v, mm, v);
      }
      for (int i = 0; i < 4; ++i) values[(s * num_targets + j) * 4 + i] = v[i];
    }
    if (out)
      for (int i = 0; i < 4; ++i) out[s * 4 + i] = ok ? secret[i] : zero[i];
    if (nerr) nerr[s] = ok ? (u32)wrong.size() : PVW_SHAMIR_UNDECODABLE;
    if (err_mask) std::fill(err_mask + s * words, err_mask + (s + 1) * words, (u64)0);
    if (ok)
      for (size_t c : wrong) {
        if (col_err) ++col_err[c];
        if (err_mask) err_mask[s * words + c / 64] |= (u64)1 << (c % 64);
      }
    volatile u64* vs = secret;
    for (int i = 0; i < 4; ++i) vs[i] = 0;
  }
  for (std::vector<u64>* v : {&y, &A, &sol, &W, &N}) {                           // as secret as the shares
    volatile u64* vp = v->data();
    for (size_t i = 0; i < v->size(); ++i) vp[i] = 0;
  }
}
int32_t pvw_shamir_reconstruct_wide_corrected_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                   const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                   uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  berlekamp_welch_wide_host(r, shares, out, nerr, col_err, err_mask);
  return PVW_OK;
}

int32_t pvw_shamir_reconstruct_wide_corrected_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                     size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                     size_t point_stride, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                     uint64_t* d_err_mask, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, d_shares, d_out));
  PVW_TRY(correct_device_checks(r));
  return corrected_device_call(c, r, d_shares, nullptr, d_out, d_nerr, d_col_err, d_err_mask, stream,
                                  "corrected reconstruction under stream capture: run a call with the same degree and count and at least as "
                                  "many secrets on this stream outside capture first (it sizes the workspace)");
}

int32_t pvw_shamir_reconstruct_wide_corrected(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                              size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                              size_t point_stride, uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  PVW_TRY(correct_device_checks(r));
  return corrected_host_call(c, r, shares, nullptr, out, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ erasures below 2^256
// The contract of 8.16 with wide elements: erased [num_secrets][W] in the layout of err_mask; with eps_s erased columns in row s
// and E_s = (r - eps_s) / 2, row s is decodable iff eps_s <= r and some F_s of degree <= t disagrees with the row in at most E_s
// of the columns that are not erased.  erased == NULL is the call of 8.20: every entry point hands such a call over as it is.

// The contract in plain C++: erasures_host over berlekamp_welch_wide_host.
static const char* const kWideErasuresUnsized =
    "wide reconstruction with erasures under stream capture: run a call with an erasure mask, the same degree and count and at least as "
    "many secrets on this stream outside capture first (it sizes the workspace)";

int32_t pvw_shamir_reconstruct_wide_erasures_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                  const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                  const uint64_t* erased, uint64_t* out, uint32_t* nerr, uint32_t* col_err,
                                                  uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_reconstruct_wide_corrected_host(plain_modulus, degree, indices, count, shares, num_secrets, secret_stride,
                                                      point_stride, out, nerr, col_err, err_mask);
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  erasures_host(r, shares, erased, out, nerr, col_err, err_mask, nullptr, 0, nullptr);
  return PVW_OK;
}
int32_t pvw_shamir_reconstruct_wide_erasures_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                    size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                    size_t point_stride, const uint64_t* d_erased, uint64_t* d_out, uint32_t* d_nerr,
                                                    uint32_t* d_col_err, uint64_t* d_err_mask, void* stream) {
  if (!d_erased)
    return pvw_shamir_reconstruct_wide_corrected_device(c, plain_modulus, degree, indices, count, d_shares, num_secrets, secret_stride,
                                                        point_stride, d_out, d_nerr, d_col_err, d_err_mask, stream);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_wide_checks(r, d_shares, d_out));
  PVW_TRY(correct_device_checks(r));
  return corrected_device_call(c, r, d_shares, d_erased, d_out, d_nerr, d_col_err, d_err_mask, stream, kWideErasuresUnsized);
}
int32_t pvw_shamir_reconstruct_wide_erasures(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                             size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                             size_t point_stride, const uint64_t* erased, uint64_t* out, uint32_t* nerr,
                                             uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_reconstruct_wide_corrected(c, plain_modulus, degree, indices, count, shares, num_secrets, secret_stride,
                                                 point_stride, out, nerr, col_err, err_mask);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(reconstruct_wide_checks(r, shares, out));
  PVW_TRY(correct_device_checks(r));
  return corrected_host_call(c, r, shares, erased, out, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ evaluation below 2^256
// The decode of 8.20 (8.21 with a mask), then values[s][j] = F_s(targets[j] + 1), four words, for every decodable row (0 for the
// others).  One decode yields out, nerr, col_err, err_mask and values; the frame is that of 8.13 with elements of four words.

// What the matching wide call refuses, in its order (values stands where it has out: out may be NULL here), then the targets.
// device: num_targets is bounded BEFORE the targets are read, so a refused count costs no walk over the array.
static int32_t evaluate_wide_checks(Reconstruct<WideCalls>& r, const void* shares, const uint64_t* targets, size_t num_targets, const void* values,
                                    bool device) {
  PVW_TRY(reconstruct_wide_checks(r, shares, values));
  if (device) PVW_TRY(correct_device_checks(r));
  if (!targets) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (num_targets == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no targets to evaluate at");
  if (device && num_targets >= ((size_t)1 << 31))
    return fail(PVW_ERR_INVALID_PARAMETERS, "num_targets must be below 2^31 on the device");
  // the point targets[j] + 1 <= 2^64 must be below p, as for the indices (reconstruct_wide_checks)
  const bool one_word = !r.p[1] && !r.p[2] && !r.p[3];
  const bool above_2_64 = r.p[2] || r.p[3] || r.p[1] > 1 || (r.p[1] == 1 && r.p[0] != 0);
  for (size_t j = 0; j < num_targets; ++j)
    if (one_word ? targets[j] >= r.p[0] - 1 : (targets[j] == ~(u64)0 && !above_2_64))
      return fail(PVW_ERR_INVALID_PARAMETERS, "target index out of range for plain_modulus");
  return PVW_OK;
}

// the points targets[j] + 1 <= 2^64 of an index form as field elements (below p: evaluate_wide_checks)
static std::vector<u64> wide_index_points(const uint64_t* targets, size_t num_targets) {
  std::vector<u64> pts(num_targets * 4, 0);
  for (size_t j = 0; j < num_targets; ++j) pts[j * 4] = targets[j] + 1, pts[j * 4 + 1] = targets[j] + 1 == 0;
  return pts;
}
int32_t pvw_shamir_evaluate_wide_corrected_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out,
                                                uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_wide_checks(r, shares, targets, num_targets, values, false));
  const std::vector<u64> pts = wide_index_points(targets, num_targets);
  berlekamp_welch_wide_host(r, shares, out, nerr, col_err, err_mask, pts.data(), num_targets, values);
  return PVW_OK;
}
int32_t pvw_shamir_evaluate_wide_erasures_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                               const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                               const uint64_t* erased, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                               uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_evaluate_wide_corrected_host(plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride,
                                                   targets, num_targets, values, out, nerr, col_err, err_mask);
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_wide_checks(r, shares, targets, num_targets, values, false));
  const std::vector<u64> pts = wide_index_points(targets, num_targets);
  erasures_host(r, shares, erased, out, nerr, col_err, err_mask, pts.data(), num_targets, values);
  return PVW_OK;
}

static const char* const kWideEvaluateUnsized =
    "wide corrected evaluation under stream capture: run a call with the same degree and count, at least as many targets and at least "
    "as many secrets on this stream outside capture first (it sizes the workspace)";
static const char* const kWideEvaluateErasuresUnsized =
    "wide evaluation with erasures under stream capture: run a call with an erasure mask, the same degree and count, at least as many "
    "targets and at least as many secrets on this stream outside capture first (it sizes the workspace)";

int32_t pvw_shamir_evaluate_wide_corrected_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                  size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                  size_t point_stride, const uint64_t* targets, size_t num_targets, uint64_t* d_values,
                                                  uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask,
                                                  void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_wide_checks(r, d_shares, targets, num_targets, d_values, true));
  return evaluate_device_call(c, r, d_shares, nullptr, EvalTargets::indices(targets), num_targets, d_values,
                              d_out, d_nerr, d_col_err, d_err_mask, stream, kWideEvaluateUnsized);
}
int32_t pvw_shamir_evaluate_wide_erasures_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                 size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                 size_t point_stride, const uint64_t* d_erased, const uint64_t* targets, size_t num_targets,
                                                 uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err,
                                                 uint64_t* d_err_mask, void* stream) {
  if (!d_erased)
    return pvw_shamir_evaluate_wide_corrected_device(c, plain_modulus, degree, indices, count, d_shares, num_secrets, secret_stride,
                                                     point_stride, targets, num_targets, d_values, d_out, d_nerr, d_col_err, d_err_mask,
                                                     stream);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_wide_checks(r, d_shares, targets, num_targets, d_values, true));
  return evaluate_device_call(c, r, d_shares, d_erased, EvalTargets::indices(targets), num_targets, d_values,
                              d_out, d_nerr, d_col_err, d_err_mask, stream, kWideEvaluateErasuresUnsized);
}

int32_t pvw_shamir_evaluate_wide_corrected(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                           const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                           const uint64_t* targets, size_t num_targets, uint64_t* values, uint64_t* out, uint32_t* nerr,
                                           uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride};
  PVW_TRY(evaluate_wide_checks(r, shares, targets, num_targets, values, true));
  return evaluate_host_call(c, r, shares, nullptr, EvalTargets::indices(targets), num_targets, values,
                            out, nerr, col_err, err_mask);
}
int32_t pvw_shamir_evaluate_wide_erasures(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                          const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                          const uint64_t* erased, const uint64_t* targets, size_t num_targets, uint64_t* values,
                                          uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!erased)
    return pvw_shamir_evaluate_wide_corrected(c, plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride,
                                              targets, num_targets, values, out, nerr, col_err, err_mask);
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, true};
  PVW_TRY(evaluate_wide_checks(r, shares, targets, num_targets, values, true));
  return evaluate_host_call(c, r, shares, erased, EvalTargets::indices(targets), num_targets, values,
                            out, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ evaluation at field points below 2^256
// The calls of 8.22 with the point of column j of `values` given as the field element points[j], a HOST array [num_points][4]
// below p in every form: 0, points above 2^64 and points that meet a column without being a target's index + 1 are legal.  The
// packed call evaluates at 0, -1, ..., -(pack - 1), where a packed row of 8.23 keeps its secrets.

// What the matching index form refuses, with its texts and in its order; then the points.  device: num_points is bounded BEFORE
// the points are walked.
static int32_t evaluate_wide_at_checks(Reconstruct<WideCalls>& r, const void* shares, const uint64_t* points, size_t num_points,
                                       const void* values, bool device) {
  PVW_TRY(reconstruct_wide_checks(r, shares, values));
  if (device) PVW_TRY(correct_device_checks(r));
  if (!points) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (num_points == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no points to evaluate at");
  if (device && num_points >= ((size_t)1 << 31)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_points must be below 2^31 on the device");
  const u64 pw[4] = {r.p[0], r.p[1], r.p[2], r.p[3]};
  for (size_t j = 0; j < num_points; ++j) {
    const u64 x[4] = {points[j * 4], points[j * 4 + 1], points[j * 4 + 2], points[j * 4 + 3]};
    if (!wide_less(x, pw)) return fail(PVW_ERR_INVALID_PARAMETERS, "point out of range for plain_modulus");
  }
  return PVW_OK;
}

// erased may be NULL in all three: the corrected call, its capture message included
int32_t pvw_shamir_evaluate_wide_erasures_at_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                  const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                  const uint64_t* erased, const uint64_t* points, size_t num_points, uint64_t* values,
                                                  uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, erased != nullptr};
  PVW_TRY(evaluate_wide_at_checks(r, shares, points, num_points, values, false));
  if (erased) erasures_host(r, shares, erased, out, nerr, col_err, err_mask, points, num_points, values);
  else berlekamp_welch_wide_host(r, shares, out, nerr, col_err, err_mask, points, num_points, values);
  return PVW_OK;
}
int32_t pvw_shamir_evaluate_wide_erasures_at_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                    size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                    size_t point_stride, const uint64_t* d_erased, const uint64_t* points,
                                                    size_t num_points, uint64_t* d_values, uint64_t* d_out, uint32_t* d_nerr,
                                                    uint32_t* d_col_err, uint64_t* d_err_mask, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, d_erased != nullptr};
  PVW_TRY(evaluate_wide_at_checks(r, d_shares, points, num_points, d_values, true));
  return evaluate_device_call(c, r, d_shares, d_erased, EvalTargets::wide_points(points), num_points, d_values, d_out, d_nerr, d_col_err,
                              d_err_mask, stream, d_erased ? kWideEvaluateErasuresUnsized : kWideEvaluateUnsized);
}
int32_t pvw_shamir_evaluate_wide_erasures_at(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                             size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                             size_t point_stride, const uint64_t* erased, const uint64_t* points, size_t num_points,
                                             uint64_t* values, uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_secrets, secret_stride, point_stride, erased != nullptr};
  PVW_TRY(evaluate_wide_at_checks(r, shares, points, num_points, values, true));
  return evaluate_host_call(c, r, shares, erased, EvalTargets::wide_points(points), num_points, values, out, nerr, col_err, err_mask);
}
int32_t pvw_shamir_evaluate_wide_corrected_at_host(const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices, size_t count,
                                                   const uint64_t* shares, size_t num_secrets, size_t secret_stride, size_t point_stride,
                                                   const uint64_t* points, size_t num_points, uint64_t* values, uint64_t* out,
                                                   uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  return pvw_shamir_evaluate_wide_erasures_at_host(plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride,
                                                   nullptr, points, num_points, values, out, nerr, col_err, err_mask);
}
int32_t pvw_shamir_evaluate_wide_corrected_at_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                                     size_t count, const uint64_t* d_shares, size_t num_secrets, size_t secret_stride,
                                                     size_t point_stride, const uint64_t* points, size_t num_points, uint64_t* d_values,
                                                     uint64_t* d_out, uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask,
                                                     void* stream) {
  return pvw_shamir_evaluate_wide_erasures_at_device(c, plain_modulus, degree, indices, count, d_shares, num_secrets, secret_stride,
                                                     point_stride, nullptr, points, num_points, d_values, d_out, d_nerr, d_col_err,
                                                     d_err_mask, stream);
}
int32_t pvw_shamir_evaluate_wide_corrected_at(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t degree, const uint64_t* indices,
                                              size_t count, const uint64_t* shares, size_t num_secrets, size_t secret_stride,
                                              size_t point_stride, const uint64_t* points, size_t num_points, uint64_t* values,
                                              uint64_t* out, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  return pvw_shamir_evaluate_wide_erasures_at(c, plain_modulus, degree, indices, count, shares, num_secrets, secret_stride, point_stride,
                                              nullptr, points, num_points, values, out, nerr, col_err, err_mask);
}

// The packed secrets in one call: a row of `degree` random coefficients and `pack` secrets is decoded at polynomial degree
// degree + pack - 1 and read at the points -m.  Refused in this order: NULL, pack, what the wide erasures call refuses at that
// degree, an index at or above p - pack (the rule of pvw_shamir_reconstruct_packed_wide: no secret point meets a column).
static int32_t packed_wide_secrets_checks(Reconstruct<WideCalls>& r, uint32_t pack, uint32_t degree, const void* shares, const void* secrets,
                                          bool device) {
  if (!r.p || !r.indices || !shares || !secrets) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (pack == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at least 1");
  if (pack > PVW_WIDE_MAX_PACK) return fail(PVW_ERR_INVALID_PARAMETERS, "pack must be at most PVW_WIDE_MAX_PACK");
  if (degree > 0xFFFFFFFFu - pack) return fail(PVW_ERR_INVALID_PARAMETERS, "degree + pack must be below 2^32");
  r.degree = degree + pack - 1;
  PVW_TRY(reconstruct_wide_checks(r, shares, secrets));
  const u64 pw[4] = {r.p[0], r.p[1], r.p[2], r.p[3]};
  for (size_t i = 0; i < r.count; ++i) {
    u64 top[4] = {r.indices[i] + pack, 0, 0, 0};           // index + pack as a wide integer
    top[1] = top[0] < r.indices[i];
    if (!wide_less(top, pw)) return fail(PVW_ERR_INVALID_PARAMETERS, "party index must be below plain_modulus - pack");
  }
  if (device) PVW_TRY(correct_device_checks(r));
  return PVW_OK;
}
static const char* const kPackedWideSecretsUnsized =
    "packed wide secrets under stream capture: run a call with the same mask or none, the same degree, pack and count and at least as "
    "many rows on this stream outside capture first (it sizes the workspace)";

int32_t pvw_shamir_packed_wide_secrets_host(const uint64_t* plain_modulus, uint32_t pack, uint32_t degree, const uint64_t* indices,
                                            size_t count, const uint64_t* shares, size_t num_rows, size_t secret_stride,
                                            size_t point_stride, const uint64_t* erased, uint64_t* secrets, uint32_t* nerr,
                                            uint32_t* col_err, uint64_t* err_mask) {
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_rows, secret_stride, point_stride, erased != nullptr};
  PVW_TRY(packed_wide_secrets_checks(r, pack, degree, shares, secrets, false));
  std::vector<u64> pts((size_t)pack * 4, 0);               // p - m, and 0 for m = 0
  for (u32 m = 1; m < pack; ++m) {
    u64 br = m;
    for (int k = 0; k < 4; ++k) {
      pts[(size_t)m * 4 + k] = plain_modulus[k] - br;
      br = plain_modulus[k] < br;
    }
  }
  if (erased) erasures_host(r, shares, erased, (u64*)nullptr, nerr, col_err, err_mask, pts.data(), pack, secrets);
  else berlekamp_welch_wide_host(r, shares, nullptr, nerr, col_err, err_mask, pts.data(), pack, secrets);
  return PVW_OK;
}
int32_t pvw_shamir_packed_wide_secrets_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t pack, uint32_t degree,
                                              const uint64_t* indices, size_t count, const uint64_t* d_shares, size_t num_rows,
                                              size_t secret_stride, size_t point_stride, const uint64_t* d_erased, uint64_t* d_secrets,
                                              uint32_t* d_nerr, uint32_t* d_col_err, uint64_t* d_err_mask, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_rows, secret_stride, point_stride, d_erased != nullptr};
  PVW_TRY(packed_wide_secrets_checks(r, pack, degree, d_shares, d_secrets, true));
  return evaluate_device_call(c, r, d_shares, d_erased, EvalTargets::packed_secrets(), pack, d_secrets, nullptr, d_nerr, d_col_err,
                              d_err_mask, stream, kPackedWideSecretsUnsized);
}
int32_t pvw_shamir_packed_wide_secrets(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t pack, uint32_t degree, const uint64_t* indices,
                                       size_t count, const uint64_t* shares, size_t num_rows, size_t secret_stride, size_t point_stride,
                                       const uint64_t* erased, uint64_t* secrets, uint32_t* nerr, uint32_t* col_err, uint64_t* err_mask) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  Reconstruct<WideCalls> r{plain_modulus, degree, indices, count, num_rows, secret_stride, point_stride, erased != nullptr};
  PVW_TRY(packed_wide_secrets_checks(r, pack, degree, shares, secrets, true));
  return evaluate_host_call(c, r, shares, erased, EvalTargets::packed_secrets(), pack, secrets, nullptr, nerr, col_err, err_mask);
}

// ------------------------------------------------------------------------ handover over a prime below 2^256
// The public arithmetic either side of one pass of int64 combinations: the weight rows (signed digits of
// lambda_{d,m} 2^(limb_bits w) mod p) and the fold of the decrypted digit plaintexts.  The host forms run the scaled step of
// pvw_wide.h (the kernels run Montgomery's product) and prefix / suffix products (the kernels run the Cauchy entries of 8.22).
static_assert(DEC_NEGATIVE == PVW_DEC_NEGATIVE && PVW_DEC_NEGATIVE == 2, "shamir_wide_from_digits_kernel tests this bit");
#define PVW_WIDE_MAX_DIGITS 33                           // ceil(257 / 8): the digits of a 256-bit prime at digit_bits = 8

static int32_t digit_bits_check(uint32_t digit_bits) {
  if (digit_bits < 8 || digit_bits > 64) return fail(PVW_ERR_INVALID_PARAMETERS, "digit_bits must be in [8, 64]");
  return PVW_OK;
}
int32_t pvw_shamir_wide_handover_shape(const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t digit_bits, uint32_t* num_limbs,
                                       uint32_t* num_digits) {
  if (!plain_modulus || !num_limbs || !num_digits) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  uint32_t nl = 0;
  PVW_TRY(wide_limb_count(m, limb_bits, &nl));
  PVW_TRY(digit_bits_check(digit_bits));
  *num_limbs = nl;
  *num_digits = wide_signed_digit_count(m.bits, digit_bits);
  return PVW_OK;
}

static int32_t signed_digits_checks(const uint64_t* p, const void* values, size_t count, uint32_t digit_bits, const void* digits, WideMod* m) {
  if (!p || ((!values || !digits) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(digit_bits_check(digit_bits));
  return wide_modulus_check(p, m);
}
int32_t pvw_shamir_wide_signed_digits_host(const uint64_t* plain_modulus, const uint64_t* values, size_t count, uint32_t digit_bits,
                                           int64_t* digits) {
  WideMod m;
  PVW_TRY(signed_digits_checks(plain_modulus, values, count, digit_bits, digits, &m));
  const u32 V = wide_signed_digit_count(m.bits, digit_bits);
  const u64 p[4] = {plain_modulus[0], plain_modulus[1], plain_modulus[2], plain_modulus[3]};
  for (size_t i = 0; i < count; ++i) {
    Wide r;
    wide_reduce(r, values + i * 4, m);
    u64 x[4];
    wide_unscale(x, r, m);
    wide_signed_digits(x, p, digit_bits, V, (i64*)digits + i * V, 1);
  }
  return PVW_OK;
}
int32_t pvw_shamir_wide_signed_digits_device(pvw_ctx* c, const uint64_t* plain_modulus, const uint64_t* d_values, size_t count,
                                             uint32_t digit_bits, int64_t* d_digits, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(signed_digits_checks(plain_modulus, d_values, count, digit_bits, d_digits, &m));
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const hipStream_t s = call_stream(c, stream);
  ProfScope ps(c, "shamir_wide_signed_digits", s);
  PVW_HIP(launch_shamir_signed_digits_wide(d_values, count, digit_bits, wide_signed_digit_count(m.bits, digit_bits), (i64*)d_digits,
                                           make_wide_mont(plain_modulus), s));
  return PVW_OK;
}

// One call's arguments behind their checks: the valid holders compacted (their indices and the holder each of them is), the
// target points resolved (NULL: the point 0)
struct HandoverWide {
  const u64* p;
  const u64* indices;
  const uint8_t* valid;
  size_t D;
  const u64* points;
  size_t T;
  u32 limb_bits, digit_bits;
  WideMod m{};
  u32 NL = 0, V = 0;
  std::vector<u64> vidx, pts;
  std::vector<u32> col;
  size_t nv() const { return vidx.size(); }
  size_t ld() const { return D * NL; }
  size_t rows() const { return T * V; }
};
// the order: NULL, no holders, the targets' count, digit_bits, no valid holder, what reconstruct_wide_checks says about the valid
// subset (a duplicate, the range, the modulus), limb_bits, a point not below p, D NL, and T V on the device
static int32_t handover_wide_checks(HandoverWide& h, const void* weights, bool device) {
  if (!h.p || !h.indices || !weights) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (h.D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no holders");
  if (h.T == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no target points");
  if (!h.points && h.T != 1) return fail(PVW_ERR_INVALID_PARAMETERS, "points == NULL is the single point 0: num_points must be 1");
  PVW_TRY(digit_bits_check(h.digit_bits));
  if (h.D >= ((size_t)1 << 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_holders x num_limbs must be below 2^32");
  for (size_t d = 0; d < h.D; ++d)
    if (!h.valid || h.valid[d]) {
      h.vidx.push_back(h.indices[d]);
      h.col.push_back((u32)d);
    }
  if (h.vidx.empty()) return fail(PVW_ERR_INVALID_PARAMETERS, "no valid holder");
  Reconstruct<WideCalls> r{h.p, 0, h.vidx.data(), h.vidx.size(), 1, 1, 1};
  PVW_TRY(reconstruct_wide_checks(r, weights, weights));
  h.m = r.m;
  PVW_TRY(wide_limb_count(h.m, h.limb_bits, &h.NL));
  h.V = wide_signed_digit_count(h.m.bits, h.digit_bits);
  h.pts.assign(h.T * 4, 0);
  if (h.points) {
    const u64 pw[4] = {h.p[0], h.p[1], h.p[2], h.p[3]};
    for (size_t j = 0; j < h.T; ++j) {
      const u64 x[4] = {h.points[j * 4], h.points[j * 4 + 1], h.points[j * 4 + 2], h.points[j * 4 + 3]};
      if (!wide_less(x, pw)) return fail(PVW_ERR_INVALID_PARAMETERS, "a target point must be below plain_modulus (the point -m is p - m)");
    }
    h.pts.assign(h.points, h.points + h.T * 4);
  }
  if (h.D * h.NL >= ((size_t)1 << 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_holders x num_limbs must be below 2^32");
  if (device && h.T * h.V >= ((size_t)1 << 31)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_points x num_digits must be below 2^31 on the device");
  return PVW_OK;
}
static void handover_wide_weights_host(const HandoverWide& h, i64* weights) {
  const WideMod& m = h.m;
  const size_t nv = h.nv(), ld = h.ld();
  const u64 p[4] = {h.p[0], h.p[1], h.p[2], h.p[3]};
  std::fill(weights, weights + h.rows() * ld, (i64)0);
  Wide one;
  {
    Wide w1;
    wide_small(w1, 1);
    wide_reduce(one, w1, m);
  }
  std::vector<u64> x(nv * 4), u(nv * 4), run(nv * 4), suf((nv + 1) * 4);
  for (size_t i = 0; i < nv; ++i) {
    const u64 xw[4] = {h.vidx[i] + 1, h.vidx[i] + 1 == 0 ? (u64)1 : (u64)0, 0, 0};
    wide_reduce(&x[i * 4], xw, m);
  }
  // u_i = 1 / prod_{c != i}(x_i - x_c): the denominators' running products, ONE inversion, the walk back
  for (size_t i = 0; i < nv; ++i) {
    Wide den, d;
    wide_set(den, one);
    for (size_t c = 0; c < nv; ++c)
      if (c != i) {
        wide_set(d, &x[i * 4]);
        wide_submod(d, &x[c * 4], m);
        wide_mulmod_scaled(den, den, d, m);
      }
    wide_set(&u[i * 4], den);
    wide_mulmod_scaled(&run[i * 4], i ? &run[(i - 1) * 4] : one, den, m);
  }
  {
    Wide inv;
    wide_invmod(inv, &run[(nv - 1) * 4], h.p, m);
    for (size_t i = nv; i-- > 0;) {
      Wide den, ui;
      wide_set(den, &u[i * 4]);
      wide_mulmod_scaled(ui, inv, i ? &run[(i - 1) * 4] : one, m);
      wide_mulmod_scaled(inv, inv, den, m);
      wide_set(&u[i * 4], ui);
    }
  }
  const u32 h0 = h.limb_bits / 2, h1 = h.limb_bits - h0;
  const u64 zero[4] = {0, 0, 0, 0};
  for (size_t j = 0; j < h.T; ++j) {
    Wide xs, d;
    wide_reduce(xs, &h.pts[j * 4], m);
    size_t coin = SIZE_MAX;
    for (size_t i = 0; i < nv; ++i)
      if (!memcmp(xs, &x[i * 4], 32)) coin = i;
    wide_set(&suf[nv * 4], one);                                 // suf[i] = prod_{c >= i}(x* - x_c)
    for (size_t i = nv; i-- > 0;) {
      wide_set(d, xs);
      wide_submod(d, &x[i * 4], m);
      wide_mulmod_scaled(&suf[i * 4], &suf[(i + 1) * 4], d, m);
    }
    Wide pre;
    wide_set(pre, one);
    for (size_t i = 0; i < nv; ++i) {
      u64 mu[4] = {0, 0, 0, 0};
      if (coin == SIZE_MAX) {
        Wide v;
        wide_mulmod_scaled(v, pre, &suf[(i + 1) * 4], m);
        wide_mulmod_scaled(mu, v, &u[i * 4], m);
        wide_set(d, xs);
        wide_submod(d, &x[i * 4], m);
        wide_mulmod_scaled(pre, pre, d, m);
      } else if (coin == i) {
        wide_set(mu, one);
      }
      i64* out = weights + j * h.V * ld + (size_t)h.col[i] * h.NL;
      for (u32 w = 0; w < h.NL; ++w) {
        u64 pl[4] = {mu[0], mu[1], mu[2], mu[3]};
        wide_shr(pl, m.shift);
        wide_signed_digits(pl, p, h.digit_bits, h.V, out + w, ld);
        wide_step(mu, 1u << h0, zero, m);
        wide_step(mu, 1u << h1, zero, m);
      }
    }
  }
}
int32_t pvw_shamir_wide_handover_weights_host(const uint64_t* plain_modulus, const uint64_t* indices, const uint8_t* valid,
                                              size_t num_holders, const uint64_t* points, size_t num_points, uint32_t limb_bits,
                                              uint32_t digit_bits, int64_t* weights) {
  HandoverWide h{plain_modulus, indices, valid, num_holders, points, num_points, limb_bits, digit_bits};
  PVW_TRY(handover_wide_checks(h, weights, false));
  handover_wide_weights_host(h, (i64*)weights);
  return PVW_OK;
}

// targets per group: a target costs a column of C, xt, scale and coin; the budget of evaluate_group
static size_t handover_wide_group(const HandoverWide& h) {
  const size_t per = (h.nv() + 2) * 32 + 4;
  size_t tg = ((size_t)64 << 20) / per;
  if (tg > 64) tg -= tg % 64;
  if (tg == 0) tg = 1;
  return tg < h.T ? tg : h.T;
}
static size_t handover_wide_ws_bytes(const HandoverWide& h) { return shamir_handover_wide_words(h.nv(), handover_wide_group(h)) * 8; }
// the weight rows into d_weights [T V][D NL] through the public block ws (handover_wide_ws_bytes); the host arrays are consumed here
static int32_t handover_wide_weights_enqueue(pvw_ctx* c, const HandoverWide& h, u64* ws, i64* d_weights, hipStream_t s) {
  ProfScope ps(c, "shamir_handover_weights_wide", s);
  const WideMont mm = make_wide_mont(h.p);
  const size_t nv = h.nv(), Tg = handover_wide_group(h);
  u64 *x = ws, *aux = x + nv * 4, *xt = aux + (nv + 1) * 4, *scale = xt + Tg * 4, *C = scale + Tg * 4;
  u32 *coin = (u32*)(C + nv * Tg * 4), *col = (u32*)(C + nv * Tg * 4 + (Tg + 1) / 2);
  PVW_HIP(launch_shamir_points_wide(h.vidx.data(), nv, x, mm, s));
  PVW_HIP(launch_shamir_column_weights_wide(x, aux, nv, mm, s));
  PVW_HIP(launch_shamir_handover_columns(h.col.data(), nv, col, s));
  PVW_HIP(launch_wipe_words((u64*)d_weights, h.rows() * h.ld(), s));
  for (size_t j0 = 0; j0 < h.T; j0 += Tg) {
    const size_t tg = h.T - j0 < Tg ? h.T - j0 : Tg;
    PVW_HIP(launch_shamir_points_from_wide(h.pts.data() + j0 * 4, tg, xt, mm, s));
    PVW_HIP(launch_shamir_cauchy_wide(x, aux, xt, scale, C, coin, nv, tg, mm, s));
    ShamirHandoverDigits a{};
    a.scale = scale, a.C = C, a.coin = coin, a.col = col;
    a.weights = d_weights + j0 * h.V * h.ld(), a.ld = h.ld();
    a.nv = (u32)nv, a.Tg = (u32)tg, a.NL = h.NL, a.V = h.V, a.limb_bits = h.limb_bits, a.digit_bits = h.digit_bits, a.m = mm;
    PVW_HIP(launch_shamir_handover_digits_wide(a, s));
  }
  return PVW_OK;
}
static const char* const kHandoverWeightsUnsized =
    "wide handover weights under stream capture: run a call with at least as many valid holders and target points on this stream "
    "outside capture first (it sizes the workspace)";
int32_t pvw_shamir_wide_handover_weights_device(pvw_ctx* c, const uint64_t* plain_modulus, const uint64_t* indices, const uint8_t* valid,
                                                size_t num_holders, const uint64_t* points, size_t num_points, uint32_t limb_bits,
                                                uint32_t digit_bits, int64_t* d_weights, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  HandoverWide h{plain_modulus, indices, valid, num_holders, points, num_points, limb_bits, digit_bits};
  PVW_TRY(handover_wide_checks(h, d_weights, true));
  const size_t need = handover_wide_ws_bytes(h);
  auto sized = [&](hipStream_t s) { return grown_capture_check(c, s, &Workspace::handover_wide_bytes, need, kHandoverWeightsUnsized); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(ws_grow(&w->handover_wide, &w->handover_wide_bytes, need, s, false));   // public: nothing to clear
    return handover_wide_weights_enqueue(c, h, w->handover_wide, (i64*)d_weights, s);
  });
}

// ------------------------------------------------------------------------ one-word handover weights from a mask
// Row j = the Lagrange weights AT (targets[j] + 1) mod p of the holders with valid[d] != 0, centred, 0 in a masked column.  The
// device form reads the mask when its kernels run, so both forms hold ALL num_holders indices to the rules of
// pvw_shamir_lagrange_weights: the order is NULL, no holders, the targets' count, the device's bounds (before an array of that
// length is read), the indices (modulus first), a target not below p.
static int32_t handover_checks(u64 p, const u64* indices, size_t D, const u64* targets, size_t T, const void* weights, bool device) {
  if (!indices || !weights) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no holders");
  if (T == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no target points");
  if (!targets && T != 1) return fail(PVW_ERR_INVALID_PARAMETERS, "targets == NULL is the single point 0: num_targets must be 1");
  if (device && D >= ((size_t)1 << 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_holders must be below 2^32 on the device");
  if (device && T >= ((size_t)1 << 31)) return fail(PVW_ERR_INVALID_PARAMETERS, "num_targets must be below 2^31 on the device");
  PVW_TRY(shamir_index_checks(p, indices, D, true));
  for (size_t j = 0; targets && j < T; ++j)
    if (targets[j] >= p) return fail(PVW_ERR_INVALID_PARAMETERS, "target index out of range for plain_modulus");
  return PVW_OK;
}
int32_t pvw_shamir_handover_weights_host(uint64_t plain_modulus, const uint64_t* indices, const uint8_t* valid, size_t num_holders,
                                         const uint64_t* targets, size_t num_targets, int64_t* weights, uint32_t* count) {
  PVW_TRY(handover_checks(plain_modulus, indices, num_holders, targets, num_targets, weights, false));
  const Mod m = shamir_mod(plain_modulus);
  std::vector<u64> vidx, z(num_targets, 0), W;
  std::vector<size_t> col;
  for (size_t d = 0; d < num_holders; ++d)
    if (!valid || valid[d]) {
      vidx.push_back(indices[d]);
      col.push_back(d);
    }
  for (size_t j = 0; targets && j < num_targets; ++j) z[j] = targets[j] + 1 == m.q ? 0 : targets[j] + 1;
  std::fill(weights, weights + num_targets * num_holders, (int64_t)0);
  if (!vidx.empty()) {
    shamir_weights_at_points(m, vidx.data(), vidx.size(), z, &W);
    for (size_t j = 0; j < num_targets; ++j)
      for (size_t i = 0; i < vidx.size(); ++i) weights[j * num_holders + col[i]] = centred(W[j * vidx.size() + i], m.q);
  }
  if (count) *count = (uint32_t)vidx.size();
  return PVW_OK;
}

// targets per group: a target costs a column of C, xt, scale and coin, within the budget of evaluate_group
static size_t handover_group(size_t D, size_t T) {
  const size_t per = (D + 2) * 8 + 4;
  size_t tg = group_budget() / per;
  if (tg > 64) tg -= tg % 64;
  if (tg == 0) tg = 1;
  return tg < T ? tg : T;
}
// The block is sized by a bound that never shrinks when D or T grow, so that a call with at least as many holders and targets
// sizes the block for every smaller one (the words of the group itself do shrink where Tg drops to the next multiple of 64).
// A group of Tg targets takes g(Tg) = 2 Tg + D Tg + ceil(Tg / 2) words, and g(Tg) <= g(T).  Where the budget B holds the group,
// Tg ((D + 2) 8 + 4) <= B gives g(Tg) <= B / 8 + 1; where it holds no target at all, Tg = 1 and g(1) = D + 3.
static size_t handover_ws_bytes(size_t D, size_t T) {
  const size_t whole = 2 * T + D * T + (T + 1) / 2, budget = group_budget() / 8 + 1;
  const size_t cap = budget > D + 3 ? budget : D + 3;
  return (2 * D + (whole < cap ? whole : cap)) * 8;
}
// the weight rows [T][D] into d_weights through the public block ws (handover_ws_bytes), and the number of valid holders into
// *d_count (may be NULL); indices and targets (NULL: the point 0) are consumed here, d_valid is read when the kernels run
static int32_t handover_weights_enqueue(pvw_ctx* c, u64 p, const u64* indices, const uint8_t* d_valid, size_t D, const u64* targets,
                                        size_t T, u64* ws, i64* d_weights, u32* d_count, hipStream_t s) {
  ProfScope ps(c, "shamir_handover_weights", s);
  const Mod m = shamir_mod(p);
  const size_t Tg = handover_group(D, T);
  const u64 zero_point = p - 1;                                    // index p - 1 is the point 0
  if (!targets) targets = &zero_point;
  u64 *x = ws, *aux = x + D, *grp = aux + D;
  PVW_HIP(launch_shamir_points(indices, D, x, s));
  PVW_HIP(launch_shamir_masked_column_weights(x, d_valid, aux, d_count, D, m, s));
  for (size_t j0 = 0; j0 < T; j0 += Tg) {
    const size_t tg = T - j0 < Tg ? T - j0 : Tg;
    PVW_HIP(launch_shamir_points(targets + j0, tg, grp, s));
    PVW_HIP(launch_shamir_handover_weights(x, aux, d_valid, grp, D, tg, d_weights + j0 * D, m, s));
  }
  return PVW_OK;
}
static const char* const kHandoverNarrowWeightsUnsized =
    "handover weights under stream capture: run a call with at least as many holders and target points on this stream outside "
    "capture first (it sizes the workspace)";
int32_t pvw_shamir_handover_weights_device(pvw_ctx* c, uint64_t plain_modulus, const uint64_t* indices, const uint8_t* d_valid,
                                           size_t num_holders, const uint64_t* targets, size_t num_targets, int64_t* d_weights,
                                           uint32_t* d_count, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(handover_checks(plain_modulus, indices, num_holders, targets, num_targets, d_weights, true));
  const size_t need = handover_ws_bytes(num_holders, num_targets);
  auto sized = [&](hipStream_t s) { return grown_capture_check(c, s, &Workspace::handover_bytes, need, kHandoverNarrowWeightsUnsized); };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(ws_grow(&w->handover, &w->handover_bytes, need, s, false));   // public: nothing to clear
    return handover_weights_enqueue(c, plain_modulus, indices, d_valid, num_holders, targets, num_targets, w->handover, (i64*)d_weights,
                                    d_count, s);
  });
}

// The holder mask from a report: valid_out[c] = 1 iff no row r has status & status_bits or noise > noise_bound at
// r * row_stride + c * col_stride.  The argument rules of pvw_shamir_erasure_mask_* (erasure_mask_checks).
int32_t pvw_shamir_valid_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound, size_t count,
                                   size_t rows, size_t row_stride, size_t col_stride, uint8_t* valid_out, uint32_t* num_valid) {
  PVW_TRY(erasure_mask_checks(status, noise, count, rows, row_stride, col_stride, valid_out));
  uint32_t nv = 0;
  for (size_t c = 0; c < count; ++c) {
    bool bad = false;
    for (size_t r = 0; r < rows && !bad; ++r) {
      const size_t off = r * row_stride + c * col_stride;
      bad = (status && (status[off] & status_bits)) || (noise && noise[off] > noise_bound);
    }
    valid_out[c] = bad ? 0 : 1;
    nv += !bad;
  }
  if (num_valid) *num_valid = nv;
  return PVW_OK;
}
int32_t pvw_shamir_valid_mask_device(pvw_ctx* c, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits, uint64_t noise_bound,
                                     size_t count, size_t rows, size_t row_stride, size_t col_stride, uint8_t* d_valid_out,
                                     uint32_t* d_num_valid, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(erasure_mask_checks(d_status, d_noise, count, rows, row_stride, col_stride, d_valid_out));
  if (count >= ((size_t)1 << 31) || rows >= ((size_t)1 << 31))
    return fail(PVW_ERR_INVALID_PARAMETERS, "count and rows must be below 2^31 on the device");
  // no scratch of its own; under capture the stream's workspace must exist already (pvw_shamir_erasure_mask_device)
  auto sized = [&](hipStream_t s) {
    return grown_capture_check(c, s, &Workspace::handover_bytes, 0,
                               "valid mask under stream capture: run a call on this stream outside capture first (it makes the stream's "
                               "workspace)");
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace*, hipStream_t s) -> int32_t {
    ProfScope ps(c, "shamir_valid_mask", s);
    PVW_HIP(launch_shamir_valid_mask(d_status, d_noise, status_bits, noise_bound, (u32)count, (u32)rows, row_stride, col_stride, d_valid_out,
                                     d_num_valid, s));
    return PVW_OK;
  });
}

static int32_t from_digits_checks(const uint64_t* p, uint32_t digit_bits, uint32_t num_digits, const void* wide, const void* status,
                                  uint32_t ww, size_t count, const void* out, const void* status_out, WideMod* m) {
  if (!p || ((!wide || !status || !out || !status_out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(digit_bits_check(digit_bits));
  if (num_digits < 1 || num_digits > PVW_WIDE_MAX_DIGITS) return fail(PVW_ERR_INVALID_PARAMETERS, "num_digits must be in [1, 33]");
  if (ww < 1 || ww > 4) return fail(PVW_ERR_INVALID_PARAMETERS, "wide_words must be in [1, 4]");
  return wide_modulus_check(p, m);
}
int32_t pvw_shamir_wide_from_digits_host(const uint64_t* plain_modulus, uint32_t digit_bits, uint32_t num_digits, const uint64_t* wide,
                                         uint32_t* status, uint32_t wide_words, size_t count, uint64_t* out, uint32_t* status_out) {
  WideMod m;
  PVW_TRY(from_digits_checks(plain_modulus, digit_bits, num_digits, wide, status, wide_words, count, out, status_out, &m));
  const u64 zero[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < count; ++i) {
    u64 acc[4] = {0, 0, 0, 0};
    u32 st = 0;
    for (u32 v = num_digits; v-- > 0;) {
      u64 mag[4] = {0, 0, 0, 0};
      for (u32 k = 0; k < wide_words; ++k) mag[k] = wide[(i * num_digits + v) * wide_words + k];
      const u32 sv = status[i * num_digits + v];
      st |= sv;
      Wide r;
      wide_reduce(r, mag, m);
      if (sv & PVW_DEC_NEGATIVE) wide_negmod(r, m);
      u32 rem = digit_bits;
      for (; rem > 31; rem -= 31) wide_step(acc, 1u << 31, zero, m);
      wide_step(acc, 1u << rem, *(const u64(*)[4])r, m);
    }
    wide_shr(acc, m.shift);
    for (int k = 0; k < 4; ++k) out[i * 4 + k] = acc[k];
    status_out[i] = st & ~(u32)PVW_DEC_NEGATIVE;
  }
  return PVW_OK;
}
int32_t pvw_shamir_wide_from_digits_device(pvw_ctx* c, const uint64_t* plain_modulus, uint32_t digit_bits, uint32_t num_digits,
                                           const uint64_t* d_wide, uint32_t* d_status, uint32_t wide_words, size_t count,
                                           uint64_t* d_out, uint32_t* d_status_out, void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(from_digits_checks(plain_modulus, digit_bits, num_digits, d_wide, d_status, wide_words, count, d_out, d_status_out, &m));
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const hipStream_t s = call_stream(c, stream);
  ProfScope ps(c, "shamir_wide_from_digits", s);
  PVW_HIP(launch_shamir_wide_from_digits(d_wide, d_status, count, num_digits, wide_words, digit_bits, d_out, d_status_out, m,
                                         make_wide_mont(plain_modulus), s));
  return PVW_OK;
}

// The mask of wide shares from a per-limb decrypt report: bit (s, c) set iff for some w < num_limbs the element at
// s * secret_stride + c * point_stride + w * limb_stride has status & status_bits or noise > noise_bound.  The checks of
// erasure_mask_checks first, in its order, then the two limb arguments.
static int32_t wide_erasure_mask_checks(const void* status, const void* noise, size_t count, size_t num_secrets, size_t secret_stride,
                                        size_t point_stride, uint32_t num_limbs, size_t limb_stride, const void* mask_out) {
  PVW_TRY(erasure_mask_checks(status, noise, count, num_secrets, secret_stride, point_stride, mask_out));
  if (num_limbs == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a share of no limbs");
  if (limb_stride == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "a stride of 0");
  return PVW_OK;
}
int32_t pvw_shamir_wide_erasure_mask_host(uint32_t* status, const uint64_t* noise, uint32_t status_bits, uint64_t noise_bound, size_t count,
                                          size_t num_secrets, size_t secret_stride, size_t point_stride, uint32_t num_limbs,
                                          size_t limb_stride, uint64_t* mask_out) {
  PVW_TRY(wide_erasure_mask_checks(status, noise, count, num_secrets, secret_stride, point_stride, num_limbs, limb_stride, mask_out));
  const size_t words = (count + 63) / 64;
  std::fill(mask_out, mask_out + num_secrets * words, (u64)0);
  for (size_t s = 0; s < num_secrets; ++s)
    for (size_t c = 0; c < count; ++c)
      for (size_t w = 0; w < num_limbs; ++w) {
        const size_t off = s * secret_stride + c * point_stride + w * limb_stride;
        if ((status && (status[off] & status_bits)) || (noise && noise[off] > noise_bound)) mask_out[s * words + c / 64] |= (u64)1 << (c % 64);
      }
  return PVW_OK;
}
int32_t pvw_shamir_wide_erasure_mask_device(pvw_ctx* c, uint32_t* d_status, const uint64_t* d_noise, uint32_t status_bits,
                                            uint64_t noise_bound, size_t count, size_t num_secrets, size_t secret_stride,
                                            size_t point_stride, uint32_t num_limbs, size_t limb_stride, uint64_t* d_mask_out,
                                            void* stream) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(wide_erasure_mask_checks(d_status, d_noise, count, num_secrets, secret_stride, point_stride, num_limbs, limb_stride, d_mask_out));
  if (count >= ((size_t)1 << 31) || num_secrets >= ((size_t)1 << 31))
    return fail(PVW_ERR_INVALID_PARAMETERS, "count and num_secrets must be below 2^31 on the device");
  // no scratch of its own; under capture the stream's workspace must exist already (pvw_shamir_erasure_mask_device)
  auto sized = [&](hipStream_t s) {
    return grown_capture_check(c, s, &Workspace::correct_wide_bytes, 0,
                               "wide erasure mask under stream capture: run a call on this stream outside capture first (it makes the "
                               "stream's workspace)");
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace*, hipStream_t s) -> int32_t {
    ProfScope ps(c, "shamir_wide_erasure_mask", s);
    PVW_HIP(launch_shamir_wide_erasure_mask(d_status, d_noise, status_bits, noise_bound, (u32)count, (u32)num_secrets, secret_stride,
                                            point_stride, num_limbs, limb_stride, d_mask_out, s));
    return PVW_OK;
  });
}

// SELF-TEST: the kernels' product on the device, out = a b mod p
int32_t pvw_selftest_shamir_wide_mul(pvw_ctx* c, const uint64_t* plain_modulus, const uint64_t* a, const uint64_t* b, size_t count,
                                     uint64_t* out) {
  if (!c || !plain_modulus || ((!a || !b || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  for (size_t i = 0; i < count; ++i) {
    u64 x[4], y[4], pp[4];
    wide_set(x, a + i * 4);
    wide_set(y, b + i * 4);
    wide_set(pp, plain_modulus);
    if (!wide_less(x, pp) || !wide_less(y, pp)) return fail(PVW_ERR_INVALID_PARAMETERS, "the product takes a, b below plain_modulus");
  }
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const WideMont mm = make_wide_mont(plain_modulus);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, count * 96));
    u64* base = (u64*)w->scratch;
    u64 *d_a = base, *d_b = base + count * 4, *d_out = base + count * 8;
    PVW_HIP(hipMemcpyAsync(d_a, a, count * 32, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(hipMemcpyAsync(d_b, b, count * 32, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(launch_shamir_wide_mul(mm, d_a, d_b, count, d_out, w->stream));
    PVW_HIP(hipMemcpyAsync(out, d_out, count * 32, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}

// ------------------------------------------------------------------------ device randomness state
// The reference draws fresh randomness on every encrypt (encryption.rs:135-167, thread_rng()).  A state on the device
// (seed S, counter c) gives calls that are captured into a graph, or queued asynchronously, the same property: the kernels
// derive call_seed(S, c + i) when they run and advance c themselves.  The handle is pvw_rnd_state, beside DealerKeys.
static thread_local uint64_t g_rnd_free_residue = 0;   // pvw_selftest_rnd_free_residue

int32_t pvw_rnd_call_seed(const uint8_t seed[32], uint64_t counter, uint8_t out[32]) {
  if (!seed || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const ChaChaKey s = make_key(seed);
  const ChaChaKey k = call_seed(s.w, counter);
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 4; ++b) out[4 * i + b] = (uint8_t)(k.w[i] >> (8 * b));
  return PVW_OK;
}

int32_t pvw_rnd_state_create(pvw_ctx* c, const uint8_t seed[32], uint64_t counter, void** out) {
  if (!c || !seed || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = nullptr;
  PVW_TRY(ensure_device(c));
  if (stream_capturing(c->stream)) return fail(PVW_ERR_INVALID_PARAMETERS, "pvw_rnd_state_create allocates: not under stream capture");
  RndState h{};
  const ChaChaKey k = make_key(seed);
  for (int i = 0; i < 8; ++i) h.seed[i] = k.w[i];
  h.counter = h.base = counter;
  pvw_rnd_state* st = new pvw_rnd_state{c->device, c->stream, nullptr};
  hipError_t e = hipMalloc((void**)&st->dev, sizeof(RndState));
  if (e == hipSuccess) e = hipMemcpyAsync(st->dev, &h, sizeof h, hipMemcpyHostToDevice, st->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(st->stream);
  memset(&h, 0, sizeof h);
  if (e != hipSuccess) {
    if (st->dev) { (void)hipMemset(st->dev, 0, sizeof(RndState)); hipFree(st->dev); }
    delete st;
    (void)hipGetLastError();
    return fail(PVW_ERR_INTERNAL, std::string("creating the randomness state failed: ") + hipGetErrorString(e));
  }
  *out = st;
  return PVW_OK;
}

int32_t pvw_rnd_state_counter(void* handle, void* stream, uint64_t* out) {
  pvw_rnd_state* st = (pvw_rnd_state*)handle;
  if (!st || !st->dev || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  hipStream_t s = stream ? (hipStream_t)stream : st->stream;
  PVW_HIP(hipSetDevice(st->device));
  if (stream_capturing(s)) return fail(PVW_ERR_INVALID_PARAMETERS, "pvw_rnd_state_counter waits for its stream: not under stream capture");
  uint64_t v = 0;
  PVW_HIP(hipMemcpyAsync(&v, &st->dev->counter, sizeof v, hipMemcpyDeviceToHost, s));
  PVW_HIP(hipStreamSynchronize(s));
  *out = v;
  return PVW_OK;
}

int32_t pvw_rnd_state_set_counter(void* handle, uint64_t counter, void* stream) {
  pvw_rnd_state* st = (pvw_rnd_state*)handle;
  if (!st || !st->dev) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  hipStream_t s = stream ? (hipStream_t)stream : st->stream;
  PVW_HIP(hipSetDevice(st->device));
  PVW_HIP(launch_rnd_set_counter(st->dev, counter, s));   // the value travels as a kernel argument: capturable, no host buffer
  return PVW_OK;
}

int32_t pvw_rnd_state_free(void* handle) {
  pvw_rnd_state* st = (pvw_rnd_state*)handle;
  if (!st) return PVW_OK;
  int32_t rc = PVW_OK;
  if (st->dev) {
    u32 back[8];
    memset(back, 0xff, sizeof back);
    if (hipSetDevice(st->device) != hipSuccess || hipMemsetAsync(st->dev, 0, sizeof(RndState), st->stream) != hipSuccess ||
        hipMemcpyAsync(back, st->dev->seed, sizeof back, hipMemcpyDeviceToHost, st->stream) != hipSuccess ||
        hipStreamSynchronize(st->stream) != hipSuccess) {
      (void)hipGetLastError();
      rc = fail(PVW_ERR_INTERNAL, "clearing the randomness state failed");
    }
    g_rnd_free_residue = 0;
    for (u32 x : back) g_rnd_free_residue += x != 0;
    hipFree(st->dev);
  }
  delete st;
  return rc;
}

int32_t pvw_selftest_rnd_free_residue(uint64_t* nonzero_words) {
  if (!nonzero_words) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *nonzero_words = g_rnd_free_residue;
  return PVW_OK;
}

// ------------------------------------------------------------------------ decode (host, integers)
static BigInt center(const BigInt& v, const pvw_ctx* c) {              // decryption.rs:140-152
  return v > c->halfQ ? v - c->Q : v;
}
static BigInt crt_lift(const pvw_ctx* c, const uint64_t* poly, u32 coeff) {
  BigInt acc;
  for (u32 i = 0; i < c->L; ++i) {
    u64 t = mulmod(poly[(size_t)i * c->l + coeff], c->crt_inv[i], c->mods[i]);
    acc = acc + c->crt_qi[i] * BigInt(t);
  }
  return acc % c->Q;
}
// the plaintext before the u64 conversion, P = centre(-z_0 - noise_0) (decryption.rs:10-53); z: the centred coefficients
static BigInt decode_plain(const pvw_ctx* c, const uint64_t* noisy, std::vector<BigInt>& z) {
  const u32 l = c->l;
  const BigInt &Q = c->Q, &D = c->delta;
  std::vector<BigInt> tmp(l), noise(l);
  z.assign(l, BigInt());
  for (u32 j = 0; j < l; ++j) z[j] = center(crt_lift(c, noisy, j), c);                  // :109-137
  for (u32 i = 0; i + 1 < l; ++i) tmp[i] = (z[i] * D - z[i + 1]).mod_floor(Q);          // :19-27
  BigInt last = tmp[0];
  for (u32 i = 1; i + 1 < l; ++i) last = (last * D + tmp[i]).mod_floor(Q);             // :30-33
  {                                                                                     // reduce_modulo_poly :154-178
    BigInt poly_const = center(last, c);
    BigInt mod_const = center(c->delta_pow.mod_floor(Q), c);
    BigInt reduced = poly_const % mod_const;
    BigInt half = mod_const / BigInt(2);
    if (reduced > half) reduced = reduced - mod_const;
    else if (reduced < -half) reduced = reduced + mod_const;
    tmp[l - 1] = reduced.mod_floor(Q);
  }
  noise[l - 1] = tmp[l - 1];
  const BigInt delta_const = center(D.mod_floor(Q), c);
  const BigInt two_delta = delta_const * BigInt(2);
  for (u32 i = l - 1; i-- > 0;) {                                                       // :44-48, divide_by_delta_rns :180-207
    BigInt p = center((noise[i + 1] - tmp[i]).mod_floor(Q), c);
    BigInt quo;
    if (!delta_const.is_zero()) {
      BigInt twice = p * BigInt(2);
      quo = p.is_negative() ? (twice - delta_const) / two_delta : (twice + delta_const) / two_delta;
    }
    noise[i] = quo.mod_floor(Q);
  }
  return center((-z[0] - noise[0]).mod_floor(Q), c);                                    // :51-53
}
static uint64_t decode_convert(const pvw_ctx* c, const BigInt& plain) {
  const BigInt& Q = c->Q;
  if (plain.is_negative()) {                                                            // :226-247
    BigInt abs = -plain;
    if (abs <= BigInt(1000)) return 0;
    BigInt pos = (plain + Q) % Q;
    return pos.fits_u64() ? pos.low_u64() : 0;
  }
  return plain.fits_u64() ? plain.low_u64() : 0;
}
static uint64_t decode_one(const pvw_ctx* c, const uint64_t* noisy) {   // decryption.rs:10-58
  std::vector<BigInt> z;
  return decode_convert(c, decode_plain(c, noisy, z));
}

int32_t pvw_decode_host(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out) {
  if (!c || ((!noisy || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const size_t P = c->poly();
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 32) nt = 32;
  if (count < 64) nt = 1;
  if (nt == 1) {
    for (size_t d = 0; d < count; ++d) out[d] = decode_one(c, noisy + d * P);
    return PVW_OK;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([=]() {
      for (size_t d = t; d < count; d += nt) out[d] = decode_one(c, noisy + d * P);
    });
  for (auto& x : th) x.join();
  return PVW_OK;
}

// checked decode on the host: residual_i = centre(-z_i - P Delta^i) by the definition, in big integers (not the
// recurrence the device runs); noise = min(max_i |residual_i|, 2^64 - 1), status = DEC_LOSSY when out is not P
// plain decode on the host, by the definition: modulus != 0: out = P mod modulus in [0, modulus); wide_words != 0:
// the low words of |P| to wide; status also says P < 0 and |P| not fitting the wide words
static void decode_checked_one(const pvw_ctx* c, const uint64_t* noisy, u64* out, u64* noise, u32* status, u64 modulus = 0,
                               u32 wide_words = 0, u64* wide = nullptr) {
  std::vector<BigInt> z;
  const BigInt plain = decode_plain(c, noisy, z);
  *out = modulus ? plain.mod_small(modulus) : decode_convert(c, plain);
  u32 st = (plain.is_negative() || !plain.fits_u64()) ? (u32)DEC_LOSSY : 0u;
  if (modulus || wide_words) {
    if (plain.is_negative()) st |= DEC_NEGATIVE;
    if (wide_words && plain.mag.size() > wide_words) st |= DEC_WIDE_TRUNCATED;
    for (u32 w = 0; w < wide_words; ++w) wide[w] = w < plain.mag.size() ? plain.mag[w] : 0;
  }
  if (status) *status = st;
  if (!noise) return;
  const BigInt sat(~(u64)0);
  BigInt dpow(1), mx;
  for (u32 i = 0; i < c->l; ++i) {
    BigInt r = center((-z[i] - plain * dpow).mod_floor(c->Q), c);
    if (r.is_negative()) r = -r;
    if (BigInt::cmp(r, mx) > 0) mx = r;
    dpow = dpow * c->delta;
  }
  *noise = BigInt::cmp(mx, sat) >= 0 ? PVW_NOISE_SAT : mx.low_u64();
}
// The report of one call from the entry point's arguments.  Its plain options are checked before any device work:
// modulus 0 (none) or 2 <= modulus < 2^62, any integer; wide_words 0 (none) or 1 .. W, W = the 64-bit words of Q; wide
// [count][wide_words] where wide_words != 0.  The checked and unchecked forms are the call with no option set.
static int32_t report_args(const pvw_ctx* c, u64* out, u64* noise, u32* status, u64 modulus, u32 wide_words, u64* wide, Report* r) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (modulus == 1 || (modulus >> 62)) return fail(PVW_ERR_INVALID_PARAMETERS, "plain modulus must be 0 (none) or in [2, 2^62)");
  if (wide_words > c->Q.mag.size()) {
    char buf[96];
    snprintf(buf, sizeof buf, "wide_words %u exceeds the %zu words of Q", wide_words, c->Q.mag.size());
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (wide_words && !wide) return fail(PVW_ERR_INVALID_PARAMETERS, "wide_words without a wide buffer");
  r->out = out, r->noise = noise, r->status = status;
  r->m = modulus ? make_mod(modulus) : Mod{0, 0, 0};
  r->ww = wide_words;
  r->wide = wide_words ? wide : nullptr;
  return PVW_OK;
}
int32_t pvw_decode_plain_host(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise,
                              uint32_t* status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out, noise, status, plain_modulus, wide_words, wide, &rep));
  if ((!noisy || !out) && count) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const size_t P = c->poly();
  unsigned nt = std::thread::hardware_concurrency();
  if (nt == 0) nt = 1;
  if (nt > 32) nt = 32;
  if (count < 64) nt = 1;
  auto run = [=](size_t d0, size_t step) {
    for (size_t d = d0; d < count; d += step)
      decode_checked_one(c, noisy + d * P, out + d, noise ? noise + d : nullptr, status ? status + d : nullptr, plain_modulus,
                         wide_words, wide_words ? wide + d * wide_words : nullptr);
  };
  if (nt == 1) {
    run(0, 1);
    return PVW_OK;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(run, (size_t)t, (size_t)nt);
  for (auto& x : th) x.join();
  return PVW_OK;
}
int32_t pvw_decode_checked_host(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise,
                                uint32_t* status) {
  if (!c) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  return pvw_decode_plain_host(c, noisy, count, out, noise, status, 0, 0, nullptr);
}

#if PVW_TUNING
// seconds per pass of `probe` (one warm-up pass first) over the resident public key section
static int32_t time_read_probe(pvw_ctx* c, uint32_t reps, double* seconds_per_pass, uint64_t* bytes_per_pass,
                               const std::function<hipError_t(size_t tiles, u64* sink, hipStream_t s)>& probe) {
  PVW_TRY(ensure_device(c));
  if (!c->dB || c->rowsB() == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no public key section resident");
  const size_t tiles = c->tiled_words(c->rowsB()) / 128;
  hipEvent_t a = nullptr, b = nullptr;
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, ((tiles + 63) / 64 + 1) * 8));
    PVW_HIP(hipEventCreate(&a));
    PVW_HIP(hipEventCreate(&b));
    PVW_HIP(probe(tiles, (u64*)w->scratch, w->stream));   // warm-up
    PVW_HIP(hipEventRecord(a, w->stream));
    for (uint32_t i = 0; i < reps; ++i) PVW_HIP(probe(tiles, (u64*)w->scratch, w->stream));
    PVW_HIP(hipEventRecord(b, w->stream));
    PVW_HIP(hipEventSynchronize(b));
    float ms = 0;
    PVW_HIP(hipEventElapsedTime(&ms, a, b));
    *seconds_per_pass = (double)ms * 1e-3 / reps;
    *bytes_per_pass = (uint64_t)tiles * 1024;
    return PVW_OK;
  });
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  return rc;
}
// MEASUREMENT AID (tuning build only, include/pvw_hip_tuning.h): seconds per pass of a read-only kernel with mac_rows' access pattern over the resident public
// key section (B-hat, tiled): what the memory system delivers to this pattern, next to what mac_rows achieves
int32_t pvw_selftest_read_bandwidth(pvw_ctx* c, uint32_t reps, double* seconds_per_pass, uint64_t* bytes_per_pass) {
  if (!c || !seconds_per_pass || !bytes_per_pass || reps == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const u32 tpw = c->k >= 64 ? (c->k / 4 / 16) * 16 : 16;           // a workgroup covers k tiles, as in mac_rows
  return time_read_probe(c, reps, seconds_per_pass, bytes_per_pass,
                         [&](size_t tiles, u64* sink, hipStream_t s) { return launch_read_probe(c->dB, tiles, tpw, sink, s); });
}
// MEASUREMENT AID: the read probe with U tiles (2U when dbuf) in flight per wave and lds_bytes of dead LDS per
// workgroup (caps the workgroups resident per CU): bandwidth against bytes in flight
int32_t pvw_tuning_read_probe(pvw_ctx* c, uint32_t reps, uint32_t u, uint32_t dbuf, uint32_t lds_bytes, double* seconds_per_pass,
                              uint64_t* bytes_per_pass) {
  if (!c || !seconds_per_pass || !bytes_per_pass || reps == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const u32 tpw = c->k >= 128 ? (c->k / 4 / 32) * 32 : 32;
  return time_read_probe(c, reps, seconds_per_pass, bytes_per_pass, [&](size_t tiles, u64* sink, hipStream_t s) {
    return launch_read_probe2(c->dB, tiles, tpw, sink, u, (dbuf & 1) != 0, lds_bytes, s, (dbuf >> 1) & 1);
  });
}
// MEASUREMENT AID: start / end stamps of the workgroups of the last mac_rows launch made with PVW_MAC_VARIANT=40 / 41
int32_t pvw_tuning_read_stamps(pvw_ctx* c, uint64_t* stamps, uint32_t* hw_id, uint32_t count) {
  if (!c || !stamps || !hw_id) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(ensure_device(c));
  PVW_HIP(hipDeviceSynchronize());
  PVW_HIP(read_stamps(stamps, hw_id, count));
  return PVW_OK;
}
#endif  // PVW_TUNING

// SELF-TEST: one i8 MFMA through the operand maps the digit-GEMM kernels assume (exact integer data)
int32_t pvw_selftest_mfma_i8(pvw_ctx* c, const int8_t* a, const int8_t* b, int32_t* out) {
  if (!c || !a || !b || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(ensure_device(c));
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(ws_scratch(w, 8192));
    char* base = (char*)w->scratch;
    PVW_HIP(hipMemcpyAsync(base, a, 1024, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(hipMemcpyAsync(base + 1024, b, 1024, hipMemcpyHostToDevice, w->stream));
    PVW_HIP(launch_mfma_probe((const signed char*)base, (const signed char*)base + 1024, (int*)(base + 2048), w->stream));
    PVW_HIP(hipMemcpyAsync(out, base + 2048, 4096, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
}

// host execution of the fixed-width decode that the GPU runs (pvw_decode.h) -- a SELF-TEST hook so
// the device algorithm can be checked on a machine without a GPU; not used by any product path.
int32_t pvw_selftest_decode_fixed(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out) {
  if (!c || ((!noisy || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const DecodeTables& t = c->dec_host;
  std::vector<u64> x(t.W + 1), y(t.W), nres(t.L);
  for (size_t d = 0; d < count; ++d)
    out[d] = decode_one_fixed(t, noisy + d * c->poly(), BN{x.data(), 1}, BN{y.data(), 1}, BN{nres.data(), 1});
  return PVW_OK;
}

// the checked form of the same: decode_one_fixed<true>, the residual recurrence on the residues, one lift a step
int32_t pvw_selftest_decode_checked(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise,
                                    uint32_t* status) {
  if (!c || ((!noisy || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const DecodeTables& t = c->dec_host;
  std::vector<u64> x(t.W + 1), y(t.W), nres(t.L);
  for (size_t d = 0; d < count; ++d)
    out[d] = decode_one_fixed<true>(t, noisy + d * c->poly(), BN{x.data(), 1}, BN{y.data(), 1}, BN{nres.data(), 1},
                                      noise ? noise + d : nullptr, status ? status + d : nullptr);
  return PVW_OK;
}

// the plain form of the same: decode_one_fixed<true, true>, the tail the fixed-width kernel runs
int32_t pvw_selftest_decode_plain(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise,
                                  uint32_t* status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out, noise, status, plain_modulus, wide_words, wide, &rep));
  if ((!noisy || !out) && count) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const PlainArgs pa = rep.plain();
  if (!rep.plain_on()) return pvw_selftest_decode_checked(c, noisy, count, out, noise, status);
  const DecodeTables& t = c->dec_host;
  std::vector<u64> x(t.W + 1), y(t.W), nres(t.L);
  for (size_t d = 0; d < count; ++d)
    out[d] = decode_one_fixed<true, true>(t, noisy + d * c->poly(), BN{x.data(), 1}, BN{y.data(), 1}, BN{nres.data(), 1},
                                            noise ? noise + d : nullptr, status ? status + d : nullptr, &pa,
                                            pa.wide_words ? wide + d * pa.wide_words : nullptr);
  return PVW_OK;
}

// SELF-TEST (host only): the short path of decode_chain_kernel restated sequentially with the SAME arithmetic (pvw_decode.h:
// garner_small, small_chain_step, small_top_*): candidates for every chain input, each confirmed on every limb; noise_{l-1}
// guessed and proven; the chain as passes to a fixed point; the plaintext from the two small values.  true + *out when every
// proof holds (the device then never touches its W-word path for this ciphertext); false when any does not (the device
// settles that part the general way; here the caller takes decode_one_fixed for the whole ciphertext -- same result).
static bool decode_one_short(const pvw_ctx* c, const u64* noisy, u64* out) {
  const DecodeTables& t = c->dec_host;
  const u32 L = t.L, l = t.ell, W = t.W;
  if (!t.gar_n || !t.sc_on || !t.hs_on || l < 3 || W < 4) return false;
  auto z = [&](u32 limb, u32 i) -> u64 { return noisy[(size_t)limb * l + i]; };
  auto res = [&](u32 limb, u32 item) -> u64 {               // tmp_item (decryption.rs:19-27) or z_0 (item == l) on one limb
    const u64 q = t.mods[limb].q;
    return item < l ? submod(mulmod_shoup(z(limb, item), t.dmod[limb], t.dmodp[limb], q), z(limb, item + 1), q) : z(limb, 0);
  };
  std::vector<u64> cand((size_t)5 * l);
  for (u32 idx = 0; idx < l; ++idx) {
    const u32 item = idx + 1 < l ? idx : l;
    u64 r[4] = {0, 0, 0, 0};
    for (u32 j = 0; j < t.gar_n; ++j) r[j] = res(j, item);
    u64* cv = &cand[(size_t)5 * idx];
    garner_small(t, r, cv);
    const bool ng = (cv[4] & 1) != 0;
    for (u32 limb = 0; limb < L; ++limb) {                    // small_confirm
      const Mod& m = t.mods[limb];
      const u64* pw = t.pow64 + (size_t)limb * W;
      u128 sum = (u128)cv[0] * pw[0] + (u128)cv[1] * pw[1];
      if (cv[2]) sum += (u128)cv[2] * pw[2];
      if (cv[3]) sum += (u128)cv[3] * pw[3];
      u64 sres = reduce128((u64)sum, (u64)(sum >> 64), m);
      if (ng && sres) sres = m.q - sres;
      if (sres != res(limb, item)) return false;
    }
    cv[4] |= 2;
  }
  // first pass of the chain: every step on a zero input
  std::vector<u64> q(l - 1), nq(l - 1);
  std::vector<char> ng(l - 1), nng(l - 1);
  const SmallVal zero{0, 0, 0, false};
  for (u32 i = 0; i + 1 < l; ++i) {
    bool n;
    if (!small_chain_step(t.sc, zero, &cand[(size_t)5 * i], q[i], n)) return false;
    ng[i] = n;
  }
  // small_top: the guess and its proof on every limb
  SmallVal top;
  if (!small_top_guess(t.sc, &cand[(size_t)5 * (l - 2)], q[l - 2], top)) return false;
  std::vector<u64> e(L);
  for (u32 limb = 0; limb < L; ++limb) {
    const u64* pw = t.pow64 + (size_t)limb * W;
    e[limb] = small_top_quotient(top, z(limb, 0), z(limb, l - 1), t.dpm[limb], t.dpm[L + limb], t.dpm[2 * L + limb], t.dpm[3 * L + limb],
                                 pw[0], pw[1], pw[2], t.mods[limb]);
  }
  for (u32 limb = 0; limb < L; ++limb)
    if (small_top_expected(e[0], t.mods[0].q, t.mods[limb]) != e[limb]) return false;
  // further passes: step i on the previous output of step i + 1 (the top step on the proven noise_{l-1})
  bool settled = false;
  for (int pass = 1; pass < 4 && !settled; ++pass) {
    settled = true;
    for (u32 i = 0; i + 1 < l; ++i) {
      const SmallVal a = i + 2 == l ? top : SmallVal{q[i + 1], 0, 0, ng[i + 1] != 0};
      bool n;
      if (!small_chain_step(t.sc, a, &cand[(size_t)5 * i], nq[i], n)) return false;
      nng[i] = n;
      if (nq[i] != q[i] || nng[i] != ng[i]) settled = false;
    }
    q = nq;
    ng = nng;
  }
  if (!settled) return false;
  // plaintext = -z_0 - noise_0 (:51-53), extract_constant_term_as_u64 (:226-247): both small, so the centred value is the integer
  const u64* z0 = &cand[(size_t)5 * (l - 1)];
  BigInt zv = BigInt::from_words(z0, 4);
  if (z0[4] & 1) zv = -zv;
  BigInt n0(q[0]);
  if (ng[0]) n0 = -n0;
  const BigInt v = -(zv + n0);
  *out = (v.neg || v.mag.size() > 1) ? 0 : (v.mag.empty() ? 0 : v.mag[0]);
  return true;
}
int32_t pvw_selftest_decode_shortcuts(const pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint8_t* short_path) {
  if (!c || ((!noisy || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const DecodeTables& t = c->dec_host;
  std::vector<u64> x(t.W + 1), y(t.W), nres(t.L);
  for (size_t d = 0; d < count; ++d) {
    const u64* nz = noisy + d * c->poly();
    const bool took = decode_one_short(c, nz, out + d);
    if (!took) out[d] = decode_one_fixed(t, nz, BN{x.data(), 1}, BN{y.data(), 1}, BN{nres.data(), 1});
    if (short_path) short_path[d] = took ? 1 : 0;
  }
  return PVW_OK;
}

// The decode of `cnt` noisy polynomials at nz (decryption.rs:116, :10-58), still in the NTT domain when `ntt_domain`.  The
// decode can transform back while it stages its input (no launch for :116), at the price of 94 instead of 79 registers.
// Taken while its workgroups (two ciphertexts each) are resident all at once anyway; beyond, and when the decode shares the
// chip with other work (`shared`), the 79-register decode runs behind a transform launch of its own.  rep: where the results
// go (device pointers; a field not asked for reaches launch_decode as NULL); wipe / wipe_bytes / wiped: as launch_decode.
static int32_t decode_tail(pvw_ctx* c, u64* nz, size_t cnt, bool ntt_domain, bool shared, hipStream_t s, const Report& rep,
                           u64* wipe = nullptr, size_t wipe_bytes = 0, bool* wiped = nullptr) {
  if (ntt_domain && (shared || (cnt + 1) / 2 > (size_t)2 * c->num_cus)) {
    ProfScope pi(c, "intt", s);
    PVW_HIP(launch_ntt(nz, cnt, true, c->dt, c->L, c->l, s));
    ntt_domain = false;
  }
  const PlainArgs pa = rep.plain();
  ProfScope ps(c, "decode", s);
  PVW_HIP(launch_decode(nz, rep.out, cnt, c->dec_dev, s, ntt_domain ? &c->dt : nullptr, wipe, wipe_bytes, wiped, rep.noise, rep.status,
                        rep.plain_on() ? &pa : nullptr));
  return PVW_OK;
}

// decode_scalar_pvw_rns on the device; checked: plus noise[d] / status[d] (either may be NULL); plain (DESIGN
// 8.8): the checked call plus the plain options
int32_t pvw_decode_plain_device(pvw_ctx* c, const uint64_t* d_noisy, size_t count, uint64_t* d_out, uint64_t* d_noise,
                                uint32_t* d_status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  if ((!d_noisy || !d_out) && count) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  // power basis in: read only
  return decode_tail(c, const_cast<u64*>(d_noisy), count, false, false, call_stream(c, stream), rep);
}
int32_t pvw_decode_checked_device(pvw_ctx* c, const uint64_t* d_noisy, size_t count, uint64_t* d_out, uint64_t* d_noise,
                                  uint32_t* d_status, void* stream) {
  return pvw_decode_plain_device(c, d_noisy, count, d_out, d_noise, d_status, 0, 0, nullptr, stream);
}
int32_t pvw_decode_device(pvw_ctx* c, const uint64_t* d_noisy, size_t count, uint64_t* d_out, void* stream) {
  return pvw_decode_checked_device(c, d_noisy, count, d_out, nullptr, nullptr, stream);
}
// host buffers in and out
int32_t pvw_decode_plain(pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise, uint32_t* status,
                         uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out, noise, status, plain_modulus, wide_words, wide, &rep));
  if ((!noisy || !out) && count) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (count == 0) return PVW_OK;
  PVW_TRY(ensure_device(c));
  Scratch sc;
  const size_t r_nz = sc.add(count * c->poly() * 8), r_rep = rep.reserve(sc, count);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    const Report dev = rep.in(sc, r_rep);
    PVW_HIP(hipMemcpyAsync(sc.at(r_nz), noisy, count * c->poly() * 8, hipMemcpyHostToDevice, w->stream));
    PVW_TRY(decode_tail(c, sc.at(r_nz), count, false, false, w->stream, dev));
    return dev.copy_to(rep, count, hipMemcpyDeviceToHost, w->stream);
  });
}
int32_t pvw_decode_checked(pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out, uint64_t* noise, uint32_t* status) {
  return pvw_decode_plain(c, noisy, count, out, noise, status, 0, 0, nullptr);
}
int32_t pvw_decode(pvw_ctx* c, const uint64_t* noisy, size_t count, uint64_t* out) {
  return pvw_decode_checked(c, noisy, count, out, nullptr, nullptr);
}

// ------------------------------------------------------------------------ decrypt
// A secret key kept on the device in the form the inner products read (NTT(sk[j]) in the ciphertext layout,
// secret_key.rs:98-112): decrypt calls that take one skip the transform of the key and the wipe behind it.  The reference's
// SecretKey lives as long as its owner does and is ZeroizeOnDrop (secret_key.rs:20-30); so does this: pvw_sk_free clears it.
struct pvw_sk {
  pvw_ctx* ctx;
  u64* shat;       // [k][L][l]
  size_t bytes;
};
// The key of one decrypt on the device: its coefficients (NTT(sk) is then made in w->rhat, marked secret and cleared behind
// the call), or a resident key's NTT(sk).  Exactly one is set.  key_coeffs / key_resident: from an entry point's argument,
// with its checks; rc is what the call returns before it does anything else.
struct KeyRef {
  const int64_t* coeffs;
  const u64* shat;
  int32_t rc;
};
static KeyRef key_coeffs(const pvw_ctx* c, const int64_t* d_sk) {
  if (!c || !d_sk) return KeyRef{nullptr, nullptr, fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument")};
  return KeyRef{d_sk, nullptr, PVW_OK};
}
static KeyRef key_resident(const pvw_ctx* c, const pvw_sk* sk) {
  if (!c || !sk || !sk->shat) return KeyRef{nullptr, nullptr, fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument")};
  if (sk->ctx != c) return KeyRef{nullptr, nullptr, fail(PVW_ERR_INVALID_PARAMETERS, "the key was loaded for another context")};
  return KeyRef{nullptr, sk->shat, PVW_OK};
}
// The checks the decrypt families share; each family calls them in the order it has always made them.
static int32_t check_dealers(size_t D, bool sum = false) {
  if (D == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "No ciphertexts provided");          // decryption.rs:286-290
  if (sum && (D >> 32)) return fail(PVW_ERR_INVALID_PARAMETERS, "a sum takes fewer than 2^32 dealers");
  return PVW_OK;
}
static int32_t check_ntt_input(uint32_t in_repr) {
  PVW_TRY(check_repr(in_repr));
  if (in_repr != PVW_REPR_NTT) return fail(PVW_ERR_INVALID_FORMAT, "device decrypt takes NTT-domain ciphertexts");
  return PVW_OK;
}

// noisy[d] = sum_j s-hat[j] (.) c1s[d][j] - c2col[d]  for D ciphertexts (decryption.rs:257-274): the inner products as one
// launch, cut into ranges of j when that gives the launch enough short workgroups (decrypt_split).  Returns in
// *ntt_domain whether d_noisy still has to be transformed back (change_representation(PowerBasis), :116): with ranges
// the pass that adds them up (decrypt_finish) does it; without, the consumer does -- the decode kernel itself
// (launch_decode with the transform tables) or launch_ntt.
static int32_t decrypt_mac_only(pvw_ctx* c, Workspace* w, const u64* d_c1s, const u64* d_c2col, size_t D, u64* d_noisy,
                                hipStream_t s, bool* ntt_domain, bool alone = true, const u64* shat = nullptr) {
  if (!shat) shat = w->rhat;                           // NTT(sk) made by this call (launch_prep); else a resident key's
  const u32 k = c->k, l = c->l, L = c->L;
  const u32 ns = decrypt_split(k, L, l, D);
  if (ns > 1) PVW_TRY(ws_grow(&w->dpart, &w->dpart_bytes, (size_t)ns * D * c->poly() * 8, s, false));
  {
    ProfScope ps(c, "decrypt_mac", s);
    PVW_HIP(launch_decrypt_mac(d_c1s, shat, d_c2col, d_noisy, c->dt, k, L, l, D, s, w->dpart, ns, alone));
  }
  *ntt_domain = ns <= 1;
  if (ns > 1) {
    ProfScope ps(c, "intt", s);
    PVW_HIP(launch_decrypt_finish(w->dpart, ns, d_c2col, d_noisy, c->dt, L, l, D, s));
  }
  return PVW_OK;
}
// decrypt_party_shares with device pointers end to end: <sk, c1> - c2, the transform back and the gadget decode of D dealer
// ciphertexts (NTT domain, on `s`); only D x u64 (and the report asked for) are produced.  Large batches are cut into
// chunks of about 2 GiB and the decode of chunk i (integer-ALU work, a few waves per CU) runs on a helper stream under the
// HBM-bound MAC of chunk i+1; `s` waits for the last decode before the call's work counts as complete.
static int32_t decrypt_batch_enqueue(pvw_ctx* c, Workspace* w, hipStream_t s, KeyRef key, const u64* d_c1s, const u64* d_c2col,
                                     size_t D, u64* d_noisy, const Report& rep) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly(), shat_bytes = (size_t)k * P * 8;
  // chunks of about 2 GiB of ciphertext (measured: at config 5 in full, 18 GB, overlapping the decode is -7 %;
  // with 0.3 GB chunks the cross-stream events cost more than the decode they hide, +29 %): below 3 GiB in all,
  // one pass on the caller's stream.  PVW_DECRYPT_CHUNK=<dealers> overrides.
  const long chunk_env = PVW_ENV_INT("PVW_DECRYPT_CHUNK", 0);   // tuning build only (read per call)
  const double total_gib = (double)D * k * P * 8 / (double)((size_t)1 << 30);
  size_t chunk = D;
  if (chunk_env >= 64) chunk = (size_t)chunk_env;
  else if (total_gib >= 3.0) chunk = (D + (size_t)(total_gib / 2.0) - 1) / (size_t)(total_gib / 2.0);
  const size_t nch = (D + chunk - 1) / chunk;
  if (!key.shat) {
    ws_mark_secret(w, w->rhat, shat_bytes);
    ProfScope ps(c, "prep", s);
    PVW_HIP(launch_prep(key.coeffs, nullptr, w->rhat, P, l, k, true, c->dt, L, l, s));   // NTT(sk[j]) once per call (secret_key.rs:98-112)
  }
  const bool overlap = nch >= 2;
  if (overlap) PVW_TRY(ws_aux(w, nch + 1));
  // one pass on one stream: the decode is the last launch to follow the inner products, and clears NTT(sk) on its way
  const bool decode_wipes = !overlap && !key.shat;
  for (size_t i = 0; i < nch; ++i) {
    const size_t d0 = i * chunk, cnt = (D - d0) < chunk ? (D - d0) : chunk;
    u64* nz = d_noisy + d0 * P;
    bool ntt_domain = false;
    PVW_TRY(decrypt_mac_only(c, w, d_c1s + d0 * k * P, d_c2col + d0 * P, cnt, nz, s, &ntt_domain, !overlap, key.shat));   // decryption.rs:257-274
    hipStream_t ds = s;
    if (overlap) {
      PVW_HIP(hipEventRecord(w->events[i], s));
      PVW_HIP(hipStreamWaitEvent(w->aux, w->events[i], 0));
      ds = w->aux;
    }
    bool by_decode = false;
    PVW_TRY(decode_tail(c, nz, cnt, ntt_domain, overlap, ds, rep.at(d0), decode_wipes ? w->rhat : nullptr,
                        decode_wipes ? shat_bytes : 0, &by_decode));
    if (by_decode) ws_mark_secret(w, w->rhat, shat_bytes, true);   // recorded as this call's wiped region, no memset
  }
  if (overlap) {
    PVW_HIP(hipEventRecord(w->events[nch], w->aux));
    PVW_HIP(hipStreamWaitEvent(s, w->events[nch], 0));
  }
  return PVW_OK;
}
// the device-pointer entry points: their argument checks, then the enqueue on the caller's stream.  checked: the
// same words in d_out, plus d_noise / d_status [D] (either may be NULL); plain: DESIGN 8.8
static int32_t decrypt_batch_device(pvw_ctx* c, KeyRef key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D, uint32_t in_repr,
                                    uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint64_t plain_modulus,
                                    uint32_t wide_words, uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(key.rc);
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  if ((!d_c1s || !d_c2col || !d_noisy || !d_out) && D) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_ntt_input(in_repr));
  PVW_TRY(check_dealers(D));
  return device_call(c, stream, [&](Workspace* w, hipStream_t s) {
    return decrypt_batch_enqueue(c, w, s, key, d_c1s, d_c2col, D, d_noisy, rep);
  });
}

int32_t pvw_decrypt_noisy_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                 size_t D, uint32_t in_repr, uint64_t* d_noisy, void* stream) {
  if (!c || !d_sk || ((!d_c1s || !d_c2col || !d_noisy) && D)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_ntt_input(in_repr));
  return device_call(c, stream, [&](Workspace* w, hipStream_t s) -> int32_t {
    const size_t P = c->poly();
    ws_mark_secret(w, w->rhat, (size_t)c->k * P * 8);           // NTT(sk), cleared behind the last launch that reads it
    {
      ProfScope ps(c, "prep", s);
      PVW_HIP(launch_prep(d_sk, nullptr, w->rhat, P, c->l, c->k, true, c->dt, c->L, c->l, s));   // secret_key.rs:98-112
    }
    bool ntt_domain = false;
    PVW_TRY(decrypt_mac_only(c, w, d_c1s, d_c2col, D, d_noisy, s, &ntt_domain));
    if (ntt_domain) {
      ProfScope ps(c, "intt", s);
      PVW_HIP(launch_ntt(d_noisy, D, true, c->dt, c->L, c->l, s));
    }
    return PVW_OK;
  });
}

// host buffers: dealers in chunks of <= 1 GiB of ciphertext, staged on the device (a POWER-basis chunk transformed there) and
// decrypted by the device path; the uploaded coefficients and NTT(sk) do not outlive the call (secret_key.rs:20-30)
static int32_t decrypt_batch_staged(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                                    uint32_t in_repr, uint64_t* out_u64, uint64_t* noisy_out, uint64_t* noise, uint32_t* status,
                                    uint64_t plain_modulus = 0, uint32_t wide_words = 0, uint64_t* wide = nullptr) {
  Report rep;
  PVW_TRY(report_args(c, out_u64, noise, status, plain_modulus, wide_words, wide, &rep));
  if (!sk) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_dealers(D));
  if (!c1s || !c2col || !out_u64) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(in_repr));
  PVW_TRY(ensure_device(c));
  const size_t k = c->k, l = c->l, P = c->poly(), per = chunk_1gib(k * P * 8, D);
  Scratch sc;
  const size_t r_sk = sc.add(k * l * 8), r_c1 = sc.add(per * k * P * 8), r_c2 = sc.add(per * P * 8), r_nz = sc.add(per * P * 8),
               r_rep = rep.reserve(sc, per);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    i64* d_sk = sc.at<i64>(r_sk);
    u64 *d_c1 = sc.at(r_c1), *d_c2 = sc.at(r_c2), *d_nz = sc.at(r_nz);
    const Report dev = rep.in(sc, r_rep);
    ws_mark_secret(w, d_sk, k * l * 8);
    PVW_HIP(hipMemcpyAsync(d_sk, sk, k * l * 8, hipMemcpyHostToDevice, w->stream));
    for (size_t d0 = 0; d0 < D; d0 += per) {
      const size_t cnt = (D - d0) < per ? (D - d0) : per;
      PVW_HIP(hipMemcpyAsync(d_c1, c1s + d0 * k * P, cnt * k * P * 8, hipMemcpyHostToDevice, w->stream));
      PVW_HIP(hipMemcpyAsync(d_c2, c2col + d0 * P, cnt * P * 8, hipMemcpyHostToDevice, w->stream));
      if (in_repr == PVW_REPR_POWER) {
        ProfScope ps(c, "ntt", w->stream);
        PVW_HIP(launch_ntt(d_c1, cnt * k, false, c->dt, c->L, c->l, w->stream));
        PVW_HIP(launch_ntt(d_c2, cnt, false, c->dt, c->L, c->l, w->stream));
      }
      PVW_TRY(decrypt_batch_enqueue(c, w, w->stream, key_coeffs(c, d_sk), d_c1, d_c2, cnt, d_nz, dev));
      PVW_TRY(dev.copy_to(rep.at(d0), cnt, hipMemcpyDeviceToHost, w->stream));
      if (noisy_out) PVW_HIP(hipMemcpyAsync(noisy_out + d0 * P, d_nz, cnt * P * 8, hipMemcpyDeviceToHost, w->stream));
    }
    return PVW_OK;
  });
}
int32_t pvw_decrypt_batch(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                          uint32_t in_repr, uint64_t* out_u64, uint64_t* noisy_out) {
  return decrypt_batch_staged(c, sk, c1s, c2col, D, in_repr, out_u64, noisy_out, nullptr, nullptr);
}
int32_t pvw_decrypt_batch_checked(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                                  uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status) {
  return decrypt_batch_staged(c, sk, c1s, c2col, D, in_repr, out_u64, nullptr, noise, status);
}
int32_t pvw_decrypt_batch_plain(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D, uint32_t in_repr,
                                uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint64_t plain_modulus, uint32_t wide_words,
                                uint64_t* wide) {
  return decrypt_batch_staged(c, sk, c1s, c2col, D, in_repr, out_u64, nullptr, noise, status, plain_modulus, wide_words, wide);
}

int32_t pvw_decrypt_batch_plain_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                       uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                       uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  return decrypt_batch_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide,
                              stream);
}
int32_t pvw_decrypt_batch_device_sk_plain(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                          uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                          uint32_t* d_status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide,
                                          void* stream) {
  return decrypt_batch_device(c, key_resident(c, key), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide,
                              stream);
}
int32_t pvw_decrypt_batch_checked_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                         uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                         void* stream) {
  return decrypt_batch_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, d_noise, d_status, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_batch_device_sk_checked(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                            uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                            uint32_t* d_status, void* stream) {
  return decrypt_batch_device(c, key_resident(c, key), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, d_noise, d_status, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_batch_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                 size_t D, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, void* stream) {
  return decrypt_batch_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, nullptr, nullptr, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_batch_device_sk(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col,
                                    size_t D, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, void* stream) {
  return decrypt_batch_device(c, key_resident(c, key), d_c1s, d_c2col, D, in_repr, d_noisy, d_out, nullptr, nullptr, 0, 0, nullptr, stream);
}
int32_t pvw_sk_load(pvw_ctx* c, const int64_t* sk, pvw_sk** out) {
  if (!c || !sk || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = nullptr;
  PVW_TRY(ensure_device(c));
  const size_t k = c->k, l = c->l, P = c->poly();
  pvw_sk* key = new pvw_sk{c, nullptr, k * P * 8};
  i64* stage = nullptr;
  hipError_t e = hipMalloc((void**)&key->shat, key->bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&stage, k * l * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(stage, sk, k * l * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_prep(stage, nullptr, key->shat, P, l, (u32)k, true, c->dt, c->L, c->l, c->stream);
  if (stage) {                                               // the uploaded coefficients do not outlive the call
    hipError_t e2 = hipMemsetAsync(stage, 0, k * l * 8, c->stream);
    if (e == hipSuccess) e = e2;
  }
  hipError_t e3 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e3;
  if (stage) hipFree(stage);
  if (e != hipSuccess) {
    if (key->shat) { hipMemset(key->shat, 0, key->bytes); hipFree(key->shat); }
    delete key;
    (void)hipGetLastError();
    return fail(PVW_ERR_INTERNAL, "loading the secret key failed");
  }
  *out = key;
  return PVW_OK;
}
// the resident key of party_index drawn from its seed (SecretKey::random, secret_key.rs:45-63): one sampled prologue family
// straight into the key's NTT form -- no coefficient buffer exists at any time
int32_t pvw_sk_load_seeded(pvw_ctx* c, const uint8_t sk_seed[32], uint32_t party_index, pvw_sk** out) {
  if (!c || !sk_seed || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = nullptr;
  PrologueBatch pb{};
  PrologueJob& js = pb.job[0];
  PVW_TRY(cbd_job(c->variance, js.sj));
  PVW_TRY(check_sk_index(c, (uint64_t)party_index + 1));
  PVW_TRY(ensure_device(c));
  const size_t k = c->k, l = c->l, P = c->poly();
  pvw_sk* key = new pvw_sk{c, nullptr, k * P * 8};
  pb.key[0] = make_key(sk_seed);
  js.sj.domain = DOM_SK; js.sj.index0 = party_index * c->k; js.sj.count = c->k;
  js.stride_poly = P; js.stride_limb = l;
  pb.njobs = 1;
  hipError_t e = hipMalloc((void**)&key->shat, key->bytes);
  js.out = key->shat;
  if (e == hipSuccess) e = launch_prologue(pb, c->dt, c->L, c->l, c->stream);
  hipError_t e3 = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = e3;
  if (e != hipSuccess) {
    if (key->shat) { hipMemset(key->shat, 0, key->bytes); hipFree(key->shat); }
    delete key;
    (void)hipGetLastError();
    return fail(PVW_ERR_INTERNAL, "loading the secret key failed");
  }
  *out = key;
  return PVW_OK;
}
int32_t pvw_sk_free(pvw_sk* key) {
  if (!key) return PVW_OK;
  int32_t rc = PVW_OK;
  if (key->shat) {
    if (key->ctx) (void)hipSetDevice(key->ctx->device);
    if (hipDeviceSynchronize() != hipSuccess || hipMemset(key->shat, 0, key->bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
      rc = fail(PVW_ERR_INTERNAL, "clearing the secret key failed");
    hipFree(key->shat);
  }
  delete key;
  return rc;
}
// ------------------------------------------------------------------------ decrypt for every party
// Every party of [lo, hi) decrypts its share of each of D dealer ciphertexts in one call: the loop over
// decrypt_party_shares (decryption.rs:281-325) that examples/pvw.rs:138-149 and tests/crypto.rs:284-287 run for all parties,
// and examples/pvw_valid_dec.rs:201-209 over a subset of dealers.  For each (limb, slot)
//   noisy[p][d] = sum_j s-hat_p[j] c1-hat_d[j] - c2-hat_d[p]      (decryption.rs:257-274)
// is a (P x k) (k x D) product: the digit GEMM of key generation with the parties' s-hat as the MFMA-tiled rows (made
// straight from the coefficients by shat_mftile) and the dealers' c1 as the digitised vectors (vec_digits reads the
// [D][k][L][l] layout as it is, after a pass that reduces the caller's words below q).  gemm_finish_decrypt subtracts c2
// and lays the noisy polynomials out as [party][dealer], the decode transforms back and decodes them in that order, and a
// 2-D copy puts the chunk's results into out[p][d].
// Fewer than PVW_DECRYPT_ALL_MIN_PARTIES parties: the GEMM pads its rows to whole workgroups and the digit tiles of every
// dealer cost the same for one party as for a thousand, so the call runs the per-party path (decrypt_mac + decode, the
// kernels of pvw_decrypt_batch) party by party instead.  Both give the words pvw_decrypt_batch gives.
// Measured crossover (profiles/r04_decrypt_all.txt, config 3, 1024 dealers, each side forced): 16 parties 2.30 ms on the
// matrix cores vs 1.82 party by party, 32 parties 2.82 vs 3.64 -- 0.114 ms per party against 1.77 + 0.033 per party: 22.
#ifndef PVW_DECRYPT_ALL_MIN_PARTIES
#define PVW_DECRYPT_ALL_MIN_PARTIES 22
#endif
static int32_t decrypt_all_checks(pvw_ctx* c, u32 lo, u32 hi, const void* sk, const void* c1s, const void* c2s, size_t D,
                                  uint32_t in_repr, const void* out) {
  if (!c || !sk || !c1s || !c2s || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_dealers(D));
  PVW_TRY(check_party_range(c, lo, hi));
  if (lo == hi) return fail(PVW_ERR_INVALID_PARAMETERS, "empty party range");
  PVW_TRY(check_repr(in_repr));
  return PVW_OK;
}
// Which side a call for NP parties and D dealers takes, its chunk sizes and its scratch, from the shape of the call alone
// (no workspace, stream or pointer): what the call takes is known before it runs (pvw_prepare, sum_capture_check).
// host: host buffers, staged in bounded pieces; stage: c1 / c2 are copied (host, or POWER-basis input: the caller's buffers
// are only read); noise / status / ww: the report asked for.  The staged report follows r_nz directly.
struct AllLayout {
  bool use_gemm = false, direct = false;
  size_t Dc = 0;                      // party by party: dealers per chunk
  size_t Dg = 0, nbg = 0, Pc = 0;     // matrix cores: dealers per group, their batches of 16, parties per chunk
  Scratch sc;
  size_t r_sk = 0, r_c1 = 0, r_c2 = 0, r_nz = 0, r_rep = 0, r_yd = 0, r_sy = 0, r_rows = 0, r_xm = 0, r_tmp = 0;
};
static AllLayout decrypt_all_layout(const pvw_ctx* c, size_t NP, size_t D, bool host, bool stage, bool noise, bool status, size_t ww) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly(), ctw = (size_t)k * P;       // ctw: words of one dealer's c1
  const long min_parties = PVW_ENV_INT("PVW_DECRYPT_ALL_MIN_PARTIES", PVW_DECRYPT_ALL_MIN_PARTIES);   // tuning build only
  AllLayout a;
  Scratch& sc = a.sc;
  a.use_gemm = min_parties > 0 && NP >= (size_t)min_parties;
  if (!a.use_gemm) {
    // dealers in chunks of <= 1 GiB of c1, each chunk's c1 shared by every party
    const size_t Dc = a.Dc = chunk_1gib(ctw * 8, D);
    a.r_sk = sc.add(host ? NP * k * l * 8 : 0), a.r_c1 = sc.add(stage ? Dc * ctw * 8 : 0), a.r_c2 = sc.add(Dc * P * 8);
    a.r_nz = sc.add(Dc * P * 8), a.r_rep = Report::reserve(sc, host ? Dc : 0, noise, status, ww);
    return a;
  }
  // Dealers in groups of up to 128 (one gemm_digits launch each; c1 of the group reduced and digitised once per party chunk,
  // <= 1 GiB with its digit tiles), parties in chunks that keep the rest below 3 GiB.
  size_t Dg = D < 128 ? D : 128;
  while (Dg > 1 && Dg * ctw * 72 > stage_budget()) Dg /= 2;     // c1 copy (8 bytes a word) + digit tiles (64)
  const size_t nbg = (Dg + 15) / 16;
  a.direct = l <= 32;                                              // s-hat straight into the tiled operand (shat_mftile)
  const size_t per_party = ctw * 8 * (a.direct ? 1 : 2) + nbg * 16 * P * 8 + Dg * P * 8 * (stage ? 2 : 1) + Dg * 8 + (host ? (size_t)k * l * 8 : 0);
  size_t Pc = 3 * stage_budget() / per_party;
  if (Pc >= NP) Pc = NP;
  else if (Pc >= PVW_GEMM_ROWS_PER_WG) Pc -= Pc % PVW_GEMM_ROWS_PER_WG;   // whole workgroups of GEMM rows
  if (Pc == 0) Pc = 1;
  a.Dg = Dg, a.nbg = nbg, a.Pc = Pc;
  a.r_c1 = sc.add(Dg * ctw * 8), a.r_yd = sc.add(yd_bytes((u32)(16 * nbg), k, L, l)), a.r_sy = sc.add(sy_bytes((u32)(16 * nbg), L, l));
  // from here on: everything derived from the keys
  a.r_sk = sc.add(host ? Pc * k * l * 8 : 0), a.r_rows = sc.add(a.direct ? 0 : Pc * ctw * 8);
  a.r_xm = sc.add(xm_words((u32)Pc, k, L, l) * 8), a.r_tmp = sc.add(nbg * gemm_tmp_words((u32)Pc, L, l) * 8);
  a.r_c2 = sc.add(stage ? Dg * Pc * P * 8 : 0), a.r_nz = sc.add(Dg * Pc * P * 8);
  a.r_rep = Report::reserve(sc, Dg * Pc, noise, status, ww);
  return a;
}
// The shape of one call, as both sides take it.  host: sk / c1s / c2s / rep are host buffers; otherwise device pointers on `s`.
// rep: [P][D], on the same side; rep_ld: results between consecutive parties when the call fills a block of
// columns of a wider report (0: D).
struct AllCall {
  u32 lo;
  size_t NP, D;
  const int64_t* sk;
  const u64 *c1s, *c2s;
  bool host, power;
  Report rep;
  size_t rep_ld = 0;
  size_t ld() const { return rep_ld ? rep_ld : D; }
};
// ---- party by party
static int32_t decrypt_all_by_party(pvw_ctx* c, Workspace* w, hipStream_t s, const AllLayout& a, const AllCall& q) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly(), ctw = (size_t)k * P, c2d = (size_t)c->n * P, D = q.D;   // c2d: words between dealers in c2s
  const hipMemcpyKind kin = q.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const Scratch& sc = a.sc;
  i64* d_sk = sc.at<i64>(a.r_sk);
  u64 *d_c1 = sc.at(a.r_c1), *d_c2 = sc.at(a.r_c2), *d_nz = sc.at(a.r_nz);
  const Report dev = q.rep.in(sc, a.r_rep);
  // key material: the uploaded coefficients, NTT(sk) (w->rhat), the noisy polynomials (m g-hat + noise), the decoded values
  // and their reports, wide words included
  sc.secret(w, a.r_sk, a.r_sk);
  ws_mark_secret(w, w->rhat, (size_t)k * P * 8);
  sc.secret(w, a.r_nz, a.r_rep + 3);
  if (q.host) PVW_HIP(hipMemcpyAsync(d_sk, q.sk, q.NP * k * l * 8, hipMemcpyHostToDevice, s));
  const i64* skd = q.host ? d_sk : q.sk;
  for (size_t d0 = 0; d0 < D; d0 += a.Dc) {
    const size_t cnt = (D - d0) < a.Dc ? (D - d0) : a.Dc;
    const u64* c1 = q.c1s + d0 * ctw;
    if (q.host || q.power) {
      PVW_HIP(hipMemcpyAsync(d_c1, c1, cnt * ctw * 8, kin, s));
      if (q.power) { ProfScope ps(c, "ntt", s); PVW_HIP(launch_ntt(d_c1, cnt * k, false, c->dt, L, l, s)); }
      c1 = d_c1;
    }
    for (size_t p = 0; p < q.NP; ++p) {
      // party lo + p's column of c2: one row of each dealer, n rows apart
      PVW_HIP(hipMemcpy2DAsync(d_c2, P * 8, q.c2s + d0 * c2d + (q.lo + p) * P, c2d * 8, P * 8, cnt, kin, s));
      if (q.power) { ProfScope ps(c, "ntt", s); PVW_HIP(launch_ntt(d_c2, cnt, false, c->dt, L, l, s)); }
      {
        ProfScope ps(c, "prep", s);
        PVW_HIP(launch_prep(skd + p * k * l, nullptr, w->rhat, P, l, k, true, c->dt, L, l, s));   // secret_key.rs:98-112
      }
      bool ntt_domain = false;
      const int32_t rm = decrypt_mac_only(c, w, c1, d_c2, cnt, d_nz, s, &ntt_domain);          // decryption.rs:257-274
      if (w->dpart && (p == 0 || rm != PVW_OK)) ws_mark_secret(w, w->dpart, w->dpart_bytes);   // range sums of s-hat c1
      PVW_TRY(rm);
      const Report to = q.rep.at(p * q.ld() + d0);
      PVW_TRY(decode_tail(c, d_nz, cnt, ntt_domain, false, s, q.host ? dev : to));
      if (q.host) PVW_TRY(dev.copy_to(to, cnt, hipMemcpyDeviceToHost, s, true));
    }
  }
  return PVW_OK;
}
// ---- matrix cores
static int32_t decrypt_all_gemm(pvw_ctx* c, Workspace* w, hipStream_t s, const AllLayout& a, const AllCall& q) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly(), ctw = (size_t)k * P, c2d = (size_t)c->n * P, D = q.D;
  const bool stage = q.host || q.power;
  const hipMemcpyKind kin = q.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind kout = q.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  const Scratch& sc = a.sc;
  u64 *d_c1 = sc.at(a.r_c1), *d_rows = sc.at(a.r_rows), *d_xm = sc.at(a.r_xm), *d_tmp = sc.at(a.r_tmp), *d_c2 = sc.at(a.r_c2),
      *d_nz = sc.at(a.r_nz);
  signed char* d_yd = sc.at<signed char>(a.r_yd);
  int* d_sy = sc.at<int>(a.r_sy);
  i64* d_sk = sc.at<i64>(a.r_sk);
  const Report dev = q.rep.in(sc, a.r_rep);
  // the uploaded coefficients, the tiled s-hat (and its rows, l = 64), the GEMM intermediate (s-hat c1), the noisy
  // polynomials, the decoded values and their reports (wide words included); the staged c2 rows share the region
  sc.secret(w, a.r_sk, a.r_rep + 3);
  for (size_t p0 = 0; p0 < q.NP; p0 += a.Pc) {
    const u32 pc = (u32)((q.NP - p0) < a.Pc ? (q.NP - p0) : a.Pc);
    const i64* skp = q.sk + p0 * k * l;
    if (q.host) {
      PVW_HIP(hipMemcpyAsync(d_sk, skp, (size_t)pc * k * l * 8, hipMemcpyHostToDevice, s));
      skp = d_sk;
    }
    {
      ProfScope ps(c, "prep", s);
      if (a.direct) {
        PVW_HIP(launch_shat_mftile(skp, nullptr, d_xm, pc, k, L, l, c->dt, s));                        // secret_key.rs:98-112
      } else {
        PVW_HIP(launch_prep(skp, nullptr, d_rows, P, l, pc * k, true, c->dt, L, l, s));
        PVW_HIP(hipMemsetAsync(d_xm, 0, xm_words(pc, k, L, l) * 8, s));
        PVW_HIP(launch_mftile(d_rows, false, d_xm, pc, k, L, l, s));
      }
    }
    for (size_t d0 = 0; d0 < D; d0 += a.Dg) {
      const u32 dg = (u32)((D - d0) < a.Dg ? (D - d0) : a.Dg);
      {
        ProfScope ps(c, "digits", s);
        const u64* c1 = q.c1s + d0 * ctw;
        if (stage) {
          PVW_HIP(hipMemcpyAsync(d_c1, c1, (size_t)dg * ctw * 8, kin, s));
          if (q.power) PVW_HIP(launch_ntt(d_c1, (size_t)dg * k, false, c->dt, L, l, s));
          c1 = d_c1;
        }
        PVW_HIP(launch_reduce_words(c1, d_c1, (size_t)dg * ctw, c->dt, L, l, s));
        // vector d = dealer: element j at d * k P + j * P + limb * l + slot
        PVW_HIP(launch_vec_digits(d_c1, ctw, d_yd, d_sy, dg, k, L, l, c->dt, s, l, P));
      }
      const u64* c2p = q.c2s + d0 * c2d + (q.lo + p0) * P;
      size_t c2v = c2d;
      if (stage) {                                                 // rows [lo + p0, lo + p0 + pc) of each dealer only
        PVW_HIP(hipMemcpy2DAsync(d_c2, (size_t)pc * P * 8, c2p, c2d * 8, (size_t)pc * P * 8, dg, kin, s));
        if (q.power) { ProfScope ps(c, "ntt", s); PVW_HIP(launch_ntt(d_c2, (size_t)dg * pc, false, c->dt, L, l, s)); }
        c2p = d_c2;
        c2v = (size_t)pc * P;
      }
      GemmSection ga{d_xm, nullptr, nullptr, d_tmp, pc, 0, 0}, gb{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
      {
        ProfScope ps(c, "gemm", s);
        PVW_HIP(launch_gemm_digits_core(ga, gb, d_yd, d_sy, c->dt, k, L, l, dg, s));
      }
      {
        ProfScope ps(c, "finish", s);
        PVW_HIP(launch_finish_decrypt(ga, d_sy, c->dt, L, l, dg, c2p, c2v, P, d_nz, s));     // decryption.rs:257-274
      }
      PVW_TRY(decode_tail(c, d_nz, (size_t)pc * dg, true, false, s, dev));
      // results[recipient][dealer] (examples/pvw.rs:157-170): the chunk's [pc][dg] block into out[p0..][d0..]
      PVW_TRY(dev.copy_block_to(q.rep.at(p0 * q.ld() + d0), pc, dg, q.ld(), kout, s));
    }
  }
  return PVW_OK;
}
static int32_t decrypt_all_run(pvw_ctx* c, Workspace* w, hipStream_t s, const AllCall& q) {
  AllLayout a = decrypt_all_layout(c, q.NP, q.D, q.host, q.host || q.power, q.rep.noise, q.rep.status, q.rep.ww);
  PVW_TRY(a.sc.take(w));
  return a.use_gemm ? decrypt_all_gemm(c, w, s, a, q) : decrypt_all_by_party(c, w, s, a, q);
}
// host buffers in and out
int32_t pvw_decrypt_all_plain(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                              size_t D, uint32_t in_repr, uint64_t* out, uint64_t* noise, uint32_t* status, uint64_t plain_modulus,
                              uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out, noise, status, plain_modulus, wide_words, wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, sk, c1s, c2s, D, in_repr, out));
  PVW_TRY(ensure_device(c));
  const AllCall q{lo, (size_t)hi - lo, D, sk, c1s, c2s, true, in_repr == PVW_REPR_POWER, rep};
  return host_call(c, [&](Workspace* w) { return decrypt_all_run(c, w, w->stream, q); });
}
int32_t pvw_decrypt_all_checked(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                size_t D, uint32_t in_repr, uint64_t* out, uint64_t* noise, uint32_t* status) {
  return pvw_decrypt_all_plain(c, lo, hi, sk, c1s, c2s, D, in_repr, out, noise, status, 0, 0, nullptr);
}
int32_t pvw_decrypt_all(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                        size_t D, uint32_t in_repr, uint64_t* out) {
  return pvw_decrypt_all_checked(c, lo, hi, sk, c1s, c2s, D, in_repr, out, nullptr, nullptr);
}
// device pointers on the caller's stream
int32_t pvw_decrypt_all_plain_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                     const uint64_t* d_c2s, size_t D, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise,
                                     uint32_t* d_status, uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, d_sk, d_c1s, d_c2s, D, in_repr, d_out));
  const AllCall q{lo, (size_t)hi - lo, D, d_sk, d_c1s, d_c2s, false, in_repr == PVW_REPR_POWER, rep};
  return device_call(c, stream, [&](Workspace* w, hipStream_t s) { return decrypt_all_run(c, w, s, q); });
}
int32_t pvw_decrypt_all_checked_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                       const uint64_t* d_c2s, size_t D, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise,
                                       uint32_t* d_status, void* stream) {
  return pvw_decrypt_all_plain_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, in_repr, d_out, d_noise, d_status, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_all_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                               const uint64_t* d_c2s, size_t D, uint32_t in_repr, uint64_t* d_out, void* stream) {
  return pvw_decrypt_all_checked_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, in_repr, d_out, nullptr, nullptr, stream);
}

// ------------------------------------------------------------------------ sums of dealers' ciphertexts
// The scheme is additively homomorphic: (sum_d c1_d, sum_d c2_d) over the valid dealers is a ciphertext of sum_d m_d under the
// same keys, so the per-party sum of shares that examples/pvw.rs:138-170 and examples/pvw_valid_dec.rs:150-209 take after D
// decrypts is one streaming pass over the ciphertexts (launch_ct_sum) and ONE decrypt.
// Workspace::sumbuf, fixed by the context's geometry (byte offsets): the slice sums of the split kernel form | the summed c1
// [k] | the summed c2 rows [n] (row r at its global position; directly behind c1, so c1 and row 0 are one run of k + 1
// polynomials) | the noisy polynomial of a single aggregate decrypt | io: the staged report of the host-buffer calls
// (Report::packed_at, sized for n parties and the wide words of a plain decode at wide_words = W).
struct SumLayout { size_t c1, c2, noisy, io, total; };
static SumLayout sum_layout(const pvw_ctx* c) {
  const size_t P8 = c->poly() * 8;
  SumLayout o;
  o.c1 = ct_sum_partial_items_max() * 16;
  o.c2 = o.c1 + (size_t)c->k * P8;
  o.noisy = o.c2 + (size_t)c->n * P8;
  o.io = o.noisy + ((P8 + 255) & ~(size_t)255);
  o.total = o.io + ((Report::packed_bytes(c->n, c->Q.mag.size()) + 255) & ~(size_t)255);
  return o;
}
// the parts of a workspace's sum buffer; a call's staged report: Report::packed_at(io, parties)
struct SumView { u64 *c1, *c2, *noisy, *io; };
static SumView sum_view(const pvw_ctx* c, const Workspace* w) {
  const SumLayout sl = sum_layout(c);
  char* b = (char*)w->sumbuf;
  return SumView{(u64*)(b + sl.c1), (u64*)(b + sl.c2), (u64*)(b + sl.noisy), (u64*)(b + sl.io)};
}
static bool sum_buffer_ready(const pvw_ctx* c, const Workspace* w) { return w && w->sumbuf_bytes >= sum_layout(c).total; }
// may hold the noisy polynomial and the results of the last aggregate decrypt: cleared before it is replaced
static int32_t sum_buffer(pvw_ctx* c, Workspace* w, hipStream_t s) {
  return ws_grow(&w->sumbuf, &w->sumbuf_bytes, sum_layout(c).total, s, true);
}
// range sums of the single-ciphertext decrypt behind a sum (decrypt_mac_only grows Workspace::dpart to this)
static size_t sum_dpart_need(const pvw_ctx* c) {
  const u32 ns = decrypt_split(c->k, c->L, c->l, 1);
  return ns > 1 ? (size_t)ns * c->poly() * 8 : 0;
}
// A device-pointer sum made under stream capture may not allocate or wait: the stream's workspace, its sum buffer and what
// the decrypt behind the sum takes (dpart_need bytes of range sums, scratch_need bytes of scratch) must be there --
// pvw_prepare(PVW_PREPARE_SUM) makes them.  Checked before the workspace is looked up and before anything is enqueued.
static int32_t sum_capture_check(pvw_ctx* c, hipStream_t s, size_t dpart_need, size_t scratch_need) {
  if (!stream_capturing(s)) return PVW_OK;
  bool ready;
  {
    std::lock_guard<std::mutex> g(c->mu);
    auto it = c->async_ws.find((void*)s);
    const Workspace* w = it == c->async_ws.end() ? nullptr : it->second;
    ready = sum_buffer_ready(c, w) && w->dpart_bytes >= dpart_need && w->scratch_bytes >= scratch_need;
  }
  if (!ready)
    return fail(PVW_ERR_INVALID_PARAMETERS, "ciphertext sum under stream capture: call pvw_prepare(PVW_PREPARE_SUM) on this stream "
                                            "first (it sizes the scratch for the context's own party range)");
  return PVW_OK;
}
// the scratch of the device-pointer decrypt behind a sum for NP parties: one NTT-domain ciphertext, the full checked report
// and wide_words of the call (a plain decode); pvw_prepare sizes for W, the most any call may ask for
static size_t decrypt_all_sum_need(const pvw_ctx* c, size_t NP, size_t wide_words) {
  return decrypt_all_layout(c, NP, 1, false, false, true, true, wide_words).sc.total;
}
// pvw_prepare(PVW_PREPARE_SUM)
static int32_t sum_prepare(pvw_ctx* c, Workspace* w, hipStream_t s) {
  PVW_TRY(sum_buffer(c, w, s));
  PVW_TRY(ws_grow(&w->dpart, &w->dpart_bytes, sum_dpart_need(c), s, false));
  const size_t need = c->party_hi > c->party_lo ? decrypt_all_sum_need(c, c->party_hi - c->party_lo, c->Q.mag.size()) : 0;
  if (w->scratch_bytes < need) PVW_HIP(hipStreamSynchronize(s));
  return ws_scratch(w, need);
}

// c2: the first polynomial summed of dealer 0 -- c2s + row_lo L l with c2_stride = n L l (whole ciphertexts), or a party's
// column with c2_stride = L l -- `rows` polynomials per dealer; c1_stride = k L l.  valid / count: device pointers (or NULL).
// weights: NULL = the sum (ct_sum_kernel); else device words [D], the weighted form of DESIGN 8.12 (ct_lincomb_kernel).
// Many combinations: m.R > 1 rows of weights, m.wstride words apart; row r's result m.c1_stride / m.c2_stride words
// behind c1_out / c2_out and its count in count[r] (ct_lincomb_many_kernel, one pass over the dealers per row tile).
struct Combos { size_t R = 1, wstride = 0, c1_stride = 0, c2_stride = 0; };
static int32_t ct_sum_enqueue(pvw_ctx* c, Workspace* w, hipStream_t s, const u64* c1s, const u64* c2, size_t c2_stride, size_t rows,
                              size_t D, const uint8_t* valid, const i64* weights, u64* c1_out, u64* c2_out, u32* count,
                              bool accumulate = false, const Combos& m = Combos()) {
  const size_t P = c->poly();
  SumRegion a, b;
  a.in = c1s; a.out = c1_out; a.stride = (size_t)c->k * P; a.items = (size_t)c->k * P / 2;
  b.in = c2; b.out = c2_out; b.stride = c2_stride; b.items = rows * P / 2;
  const size_t items = a.items + b.items;
  u32 ns = ct_sum_slices(items, D);
  if ((size_t)ns * items > ct_sum_partial_items_max()) ns = (u32)(ct_sum_partial_items_max() / items);   // a forced count (tuning build)
  if (weights && m.R > 1) {                                        // a row tile's slice planes share the partial region
    const size_t tile = ct_lincomb_many_tile(items, ns);
    if ((size_t)ns * tile * items > ct_sum_partial_items_max()) ns = (u32)(ct_sum_partial_items_max() / (tile * items));
    ProfScope ps(c, "ct_lincomb_many", s);
    PVW_HIP(launch_ct_lincomb_many(a, b, m.c1_stride, m.c2_stride, valid, weights, m.wstride, m.R, D, c->dt, c->L, c->l,
                                   ns > 1 ? w->sumbuf : nullptr, ns, accumulate, count, s));
    return PVW_OK;
  }
  if (weights) {                                                   // the weighted form: weights device words [D]
    ProfScope ps(c, "ct_lincomb", s);
    PVW_HIP(launch_ct_lincomb(a, b, valid, weights, D, c->dt, c->L, c->l, ns > 1 ? w->sumbuf : nullptr, ns, accumulate, count, s));
    return PVW_OK;
  }
  ProfScope ps(c, "ct_sum", s);
  PVW_HIP(launch_ct_sum(a, b, valid, D, c->dt, c->L, c->l, ns > 1 ? w->sumbuf : nullptr, ns, accumulate, count, s));
  return PVW_OK;
}
// a dealer takes part when it is valid and, in the weighted form (weights != NULL), its weight is not 0
static bool takes_part(const uint8_t* valid, const i64* weights, size_t d) {
  return (!valid || valid[d]) && (!weights || weights[d] != 0);
}
// ... in at least one of the R combinations, weights [R][D]
static bool takes_part_any(const uint8_t* valid, const i64* weights, size_t d, size_t R, size_t D) {
  for (size_t r = 0; r < R; ++r)
    if (takes_part(valid, weights ? weights + r * D : nullptr, d)) return true;
  return false;
}
static size_t count_valid_any(const uint8_t* valid, const i64* weights, size_t D, size_t R) {
  size_t nv = 0;
  for (size_t d = 0; d < D; ++d) nv += takes_part_any(valid, weights, d, R, D);
  return nv;
}
static size_t count_valid(const uint8_t* valid, const i64* weights, size_t D) {
  if (!valid && !weights) return D;
  size_t nv = 0;
  for (size_t d = 0; d < D; ++d) nv += takes_part(valid, weights, d);
  return nv;
}
static int32_t no_valid_dealer(size_t D, const i64* weights) {
  char buf[144];
  if (weights)
    snprintf(buf, sizeof buf, "No participating dealer (valid, weight not 0) among the %zu ciphertexts: expected at least 1, got 0", D);
  else
    snprintf(buf, sizeof buf, "No valid dealer among the %zu ciphertexts: expected at least 1, got 0", D);
  return fail(PVW_ERR_INSUFFICIENT_DATA, buf);
}
// host buffers: runs of valid dealers are copied next to each other into st_c1 [per][k] / st_c2 [per][rows] and every full
// piece is summed into d_c1_out / d_c2_out (the first piece stores, the later ones add); masked-out dealers are not copied.
// The weighted form (weights != NULL, host words [D]): the dealers that take part are staged, and the weights of the staged
// runs travel with each piece into st_w [per].  Many combinations (R > 1, weights [R][D]): a dealer is staged when
// it takes part in at least one row, so the ciphertexts cross once whatever R is; the weights travel as st_w [R][per], and row
// r's result lies c1_ostride / c2_ostride words behind d_c1_out / d_c2_out.
static int32_t ct_sum_staged(pvw_ctx* c, Workspace* w, u64* st_c1, u64* st_c2, size_t per, const u64* c1s, const u64* c2,
                             size_t c2_stride, size_t rows, size_t D, const uint8_t* valid, const i64* weights, i64* st_w,
                             u64* d_c1_out, u64* d_c2_out, size_t R = 1, size_t c1_ostride = 0, size_t c2_ostride = 0) {
  const size_t P = c->poly(), ctw = (size_t)c->k * P;
  hipStream_t s = w->stream;
  size_t fill = 0;
  bool first = true;
  auto flush = [&]() -> int32_t {
    if (!fill) return PVW_OK;
    PVW_TRY(ct_sum_enqueue(c, w, s, st_c1, st_c2, rows * P, rows, fill, nullptr, weights ? st_w : nullptr, d_c1_out, d_c2_out, nullptr,
                           !first, Combos{R, per, c1_ostride, c2_ostride}));
    first = false;
    fill = 0;
    return PVW_OK;
  };
  for (size_t d = 0; d < D;) {
    if (!takes_part_any(valid, weights, d, R, D)) { ++d; continue; }
    size_t run = 1;
    while (d + run < D && fill + run < per && takes_part_any(valid, weights, d + run, R, D)) ++run;
    if (weights && R == 1) PVW_HIP(hipMemcpyAsync(st_w + fill, weights + d, run * 8, hipMemcpyHostToDevice, s));
    if (weights && R > 1) PVW_HIP(hipMemcpy2DAsync(st_w + fill, per * 8, weights + d, D * 8, run * 8, R, hipMemcpyHostToDevice, s));
    PVW_HIP(hipMemcpyAsync(st_c1 + fill * ctw, c1s + d * ctw, run * ctw * 8, hipMemcpyHostToDevice, s));
    PVW_HIP(hipMemcpy2DAsync(st_c2 + fill * rows * P, rows * P * 8, c2 + d * c2_stride, c2_stride * 8, rows * P * 8, run,
                             hipMemcpyHostToDevice, s));
    fill += run;
    d += run;
    if (fill == per) PVW_TRY(flush());
  }
  return flush();
}

static int32_t ct_sum_checks(const pvw_ctx* c, const void* c1s, const void* c2s, size_t D, u32 lo, u32 hi, const void* c1_out,
                             const void* c2_out) {
  if (!c || !c1s || !c2s || !c1_out || !c2_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_dealers(D, true));
  if (lo > hi) return fail(PVW_ERR_INVALID_PARAMETERS, "row_lo > row_hi");
  if (hi > c->n) {
    char buf[96];
    snprintf(buf, sizeof buf, "Row index %u exceeds maximum %u", hi - 1, c->n - 1);
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  if (lo == hi) return fail(PVW_ERR_INVALID_PARAMETERS, "empty row range");
  return PVW_OK;
}
// The weighted calls are the sum calls with the kernel exchanged: every family below has ONE body that takes
// `weights` (NULL: the sum), and NULL weights at a pvw_*lincomb* entry is refused in front of it.
static int32_t need_weights(const void* weights) {
  return weights ? (int32_t)PVW_OK : fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
}
// Not a device_call: the sum marks no key material, and device_end would drain the stream of a call that failed.
static int32_t ct_sum_device(pvw_ctx* c, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t D, const uint8_t* d_valid,
                             const i64* d_weights, uint32_t lo, uint32_t hi, uint64_t* d_c1_out, uint64_t* d_c2_out, uint32_t* d_count,
                             void* stream) {
  PVW_TRY(ct_sum_checks(c, d_c1s, d_c2s, D, lo, hi, d_c1_out, d_c2_out));
  PVW_TRY(ensure_device(c));
  hipStream_t s = call_stream(c, stream);
  PVW_TRY(sum_capture_check(c, s, 0, 0));
  Workspace* w;
  PVW_TRY(ws_for_stream(c, s, &w));
  PVW_TRY(sum_buffer(c, w, s));
  const size_t P = c->poly();
  return ct_sum_enqueue(c, w, s, d_c1s, d_c2s + (size_t)lo * P, (size_t)c->n * P, hi - lo, D, d_valid, d_weights, d_c1_out, d_c2_out,
                        d_count);
}
int32_t pvw_ct_sum_device(pvw_ctx* c, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, uint32_t lo,
                          uint32_t hi, uint64_t* d_c1_out, uint64_t* d_c2_out, uint32_t* d_count, void* stream) {
  return ct_sum_device(c, d_c1s, d_c2s, D, d_valid, nullptr, lo, hi, d_c1_out, d_c2_out, d_count, stream);
}
int32_t pvw_ct_lincomb_device(pvw_ctx* c, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t D, const uint8_t* d_valid,
                              const int64_t* d_weights, uint32_t lo, uint32_t hi, uint64_t* d_c1_out, uint64_t* d_c2_out,
                              uint32_t* d_count, void* stream) {
  PVW_TRY(need_weights(d_weights));
  return ct_sum_device(c, d_c1s, d_c2s, D, d_valid, d_weights, lo, hi, d_c1_out, d_c2_out, d_count, stream);
}
static int32_t ct_sum_hostbuf(pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid, const i64* weights,
                              uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* count) {
  PVW_TRY(ct_sum_checks(c, c1s, c2s, D, lo, hi, c1_out, c2_out));
  const size_t nv = count_valid(valid, weights, D);
  if (nv == 0) return no_valid_dealer(D, weights);
  PVW_TRY(ensure_device(c));
  const size_t P = c->poly(), k = c->k, rows = hi - lo, per = chunk_1gib((k + rows) * P * 8, nv);
  Scratch sc;
  const size_t r_c1 = sc.add(per * k * P * 8), r_c2 = sc.add(per * rows * P * 8), r_w = sc.add(weights ? per * 8 : 0);
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_TRY(sum_buffer(c, w, w->stream));
    const SumView v = sum_view(c, w);
    PVW_TRY(ct_sum_staged(c, w, sc.at(r_c1), sc.at(r_c2), per, c1s, c2s + (size_t)lo * P, (size_t)c->n * P, rows, D, valid, weights,
                          sc.at<i64>(r_w), v.c1, v.c2));
    PVW_HIP(hipMemcpyAsync(c1_out, v.c1, k * P * 8, hipMemcpyDeviceToHost, w->stream));
    PVW_HIP(hipMemcpyAsync(c2_out, v.c2, rows * P * 8, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
  if (rc == PVW_OK && count) *count = (uint32_t)nv;
  return rc;
}
int32_t pvw_ct_sum(pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid, uint32_t lo, uint32_t hi,
                   uint64_t* c1_out, uint64_t* c2_out, uint32_t* count) {
  return ct_sum_hostbuf(c, c1s, c2s, D, valid, nullptr, lo, hi, c1_out, c2_out, count);
}
int32_t pvw_ct_lincomb(pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid, const int64_t* weights,
                       uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* count) {
  PVW_TRY(need_weights(weights));
  return ct_sum_hostbuf(c, c1s, c2s, D, valid, weights, lo, hi, c1_out, c2_out, count);
}
// the same function in plain loops (no GPU): a 128-bit sum per word, one Barrett step at the end
int32_t pvw_ct_sum_host(const pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid, uint32_t lo,
                        uint32_t hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* count) {
  PVW_TRY(ct_sum_checks(c, c1s, c2s, D, lo, hi, c1_out, c2_out));
  const size_t nv = count_valid(valid, nullptr, D);
  if (nv == 0) return no_valid_dealer(D, nullptr);
  const size_t P = c->poly(), l = c->l;
  auto region = [&](const u64* in, size_t stride, size_t words, u64* out) {
    for (size_t i = 0; i < words; ++i) {
      u128 acc = 0;
      for (size_t d = 0; d < D; ++d)
        if (!valid || valid[d]) acc += in[d * stride + i];
      out[i] = reduce128((u64)acc, (u64)(acc >> 64), c->mods[(i % P) / l]);
    }
  };
  region(c1s, (size_t)c->k * P, (size_t)c->k * P, c1_out);
  region(c2s + (size_t)lo * P, (size_t)c->n * P, (size_t)(hi - lo) * P, c2_out);
  if (count) *count = (uint32_t)nv;
  return PVW_OK;
}
// the weighted form by its definition (no GPU): signed_residue of the weight, mulmod by the word, addmod
static void ct_lincomb_host_row(const pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid,
                                const int64_t* weights, uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out) {
  const size_t P = c->poly(), l = c->l;
  auto region = [&](const u64* in, size_t stride, size_t words, u64* out) {
    for (size_t i = 0; i < words; ++i) {
      const Mod& m = c->mods[(i % P) / l];
      u64 acc = 0;
      for (size_t d = 0; d < D; ++d)
        if (takes_part(valid, weights, d)) acc = addmod(acc, mulmod(signed_residue(weights[d], m), in[d * stride + i], m), m.q);
      out[i] = acc;
    }
  };
  region(c1s, (size_t)c->k * P, (size_t)c->k * P, c1_out);
  region(c2s + (size_t)lo * P, (size_t)c->n * P, (size_t)(hi - lo) * P, c2_out);
}
int32_t pvw_ct_lincomb_host(const pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid,
                            const int64_t* weights, uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* count) {
  PVW_TRY(need_weights(weights));
  PVW_TRY(ct_sum_checks(c, c1s, c2s, D, lo, hi, c1_out, c2_out));
  const size_t nv = count_valid(valid, weights, D);
  if (nv == 0) return no_valid_dealer(D, weights);
  ct_lincomb_host_row(c, c1s, c2s, D, valid, weights, lo, hi, c1_out, c2_out);
  if (count) *count = (uint32_t)nv;
  return PVW_OK;
}

// ---- many combinations of the same dealers' ciphertexts: R rows of weights [R][D], row r's result at
// c1_out [r][k] / c2_out [r][row_hi - row_lo] and its participants in counts[r].  R = 1 is the call above, through its own path.
static int32_t combos_check(size_t R, bool device) {
  if (R == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "num_combos must be at least 1");
  if (device && R >> 31) return fail(PVW_ERR_INVALID_PARAMETERS, "num_combos must be below 2^31 on the device");
  return PVW_OK;
}
static void combo_counts(const uint8_t* valid, const i64* weights, size_t D, size_t R, uint32_t* counts) {
  for (size_t r = 0; counts && r < R; ++r) counts[r] = (uint32_t)count_valid(valid, weights + r * D, D);
}
// the definition: the loop of pvw_ct_lincomb_host over the rows (a row nobody takes part in: zeros)
int32_t pvw_ct_lincomb_many_host(const pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid,
                                 const int64_t* weights, size_t R, uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out,
                                 uint32_t* counts) {
  PVW_TRY(need_weights(weights));
  PVW_TRY(ct_sum_checks(c, c1s, c2s, D, lo, hi, c1_out, c2_out));
  PVW_TRY(combos_check(R, false));
  if (count_valid_any(valid, weights, D, R) == 0) return no_valid_dealer(D, weights);
  const size_t P = c->poly();
  for (size_t r = 0; r < R; ++r)
    ct_lincomb_host_row(c, c1s, c2s, D, valid, weights + r * D, lo, hi, c1_out + r * c->k * P, c2_out + r * (hi - lo) * P);
  combo_counts(valid, weights, D, R, counts);
  return PVW_OK;
}
int32_t pvw_ct_lincomb_many_device(pvw_ctx* c, const uint64_t* d_c1s, const uint64_t* d_c2s, size_t D, const uint8_t* d_valid,
                                   const int64_t* d_weights, size_t R, uint32_t lo, uint32_t hi, uint64_t* d_c1_out,
                                   uint64_t* d_c2_out, uint32_t* d_counts, void* stream) {
  PVW_TRY(need_weights(d_weights));
  PVW_TRY(ct_sum_checks(c, d_c1s, d_c2s, D, lo, hi, d_c1_out, d_c2_out));
  PVW_TRY(combos_check(R, true));
  if (R == 1) return ct_sum_device(c, d_c1s, d_c2s, D, d_valid, d_weights, lo, hi, d_c1_out, d_c2_out, d_counts, stream);
  PVW_TRY(ensure_device(c));
  hipStream_t s = call_stream(c, stream);
  PVW_TRY(sum_capture_check(c, s, 0, 0));
  Workspace* w;
  PVW_TRY(ws_for_stream(c, s, &w));
  PVW_TRY(sum_buffer(c, w, s));
  const size_t P = c->poly(), rows = hi - lo;
  return ct_sum_enqueue(c, w, s, d_c1s, d_c2s + (size_t)lo * P, (size_t)c->n * P, rows, D, d_valid, d_weights, d_c1_out, d_c2_out,
                        d_counts, false, Combos{R, D, (size_t)c->k * P, rows * P});
}
// host buffers: the participating dealers (of any row) are staged once, the R results leave through the stream's scratch
int32_t pvw_ct_lincomb_many(pvw_ctx* c, const uint64_t* c1s, const uint64_t* c2s, size_t D, const uint8_t* valid, const int64_t* weights,
                            size_t R, uint32_t lo, uint32_t hi, uint64_t* c1_out, uint64_t* c2_out, uint32_t* counts) {
  PVW_TRY(need_weights(weights));
  PVW_TRY(ct_sum_checks(c, c1s, c2s, D, lo, hi, c1_out, c2_out));
  PVW_TRY(combos_check(R, false));
  if (R == 1) return ct_sum_hostbuf(c, c1s, c2s, D, valid, weights, lo, hi, c1_out, c2_out, counts);
  const size_t nv = count_valid_any(valid, weights, D, R);
  if (nv == 0) return no_valid_dealer(D, weights);
  PVW_TRY(ensure_device(c));
  const size_t P = c->poly(), k = c->k, rows = hi - lo, per = chunk_1gib((k + rows) * P * 8, nv);
  Scratch sc;
  const size_t r_c1 = sc.add(per * k * P * 8), r_c2 = sc.add(per * rows * P * 8), r_w = sc.add(R * per * 8);
  const size_t r_o1 = sc.add(R * k * P * 8), r_o2 = sc.add(R * rows * P * 8);
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_TRY(sum_buffer(c, w, w->stream));
    PVW_TRY(ct_sum_staged(c, w, sc.at(r_c1), sc.at(r_c2), per, c1s, c2s + (size_t)lo * P, (size_t)c->n * P, rows, D, valid, weights,
                          sc.at<i64>(r_w), sc.at(r_o1), sc.at(r_o2), R, k * P, rows * P));
    PVW_HIP(hipMemcpyAsync(c1_out, sc.at(r_o1), R * k * P * 8, hipMemcpyDeviceToHost, w->stream));
    PVW_HIP(hipMemcpyAsync(c2_out, sc.at(r_o2), R * rows * P * 8, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
  if (rc == PVW_OK) combo_counts(valid, weights, D, R, counts);
  return rc;
}

// One party's aggregate share.  The summed ciphertext sits in the sum buffer (c1 | the column's sum: k + 1 polynomials in one
// run, public); this is the rest: a POWER-basis sum is transformed there, then the single-ciphertext decrypt and its checked
// decode (decrypt_batch_enqueue with D = 1: the split decrypt_mac + decrypt_finish + the checked decode chain).
static int32_t decrypt_sum_tail(pvw_ctx* c, Workspace* w, hipStream_t s, KeyRef key, uint32_t in_repr, u64* d_noisy, const Report& rep) {
  const SumView v = sum_view(c, w);
  if (in_repr == PVW_REPR_POWER) {
    ProfScope ps(c, "ntt", s);
    PVW_HIP(launch_ntt(v.c1, (size_t)c->k + 1, false, c->dt, c->L, c->l, s));
  }
  if (d_noisy) return decrypt_batch_enqueue(c, w, s, key, v.c1, v.c2, 1, d_noisy, rep);
  // m g + noise of the aggregate is the key holder's: kept in the sum buffer and cleared by a launch right behind the decode
  // (a kernel, so that a captured call clears it on every replay in order); a call that fails on the way leaves it marked
  ws_mark_secret(w, v.noisy, c->poly() * 8);
  PVW_TRY(decrypt_batch_enqueue(c, w, s, key, v.c1, v.c2, 1, v.noisy, rep));
  PVW_HIP(launch_wipe_words(v.noisy, c->poly(), s));
  ws_mark_secret(w, v.noisy, c->poly() * 8, true);
  return PVW_OK;
}
// shared by the host-buffer and device-pointer forms; any_null: of the family's own pointer arguments
static int32_t decrypt_sum_checks(bool any_null, size_t D, uint32_t in_repr) {
  if (any_null) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_dealers(D, true));
  return check_repr(in_repr);
}
// device pointers; checked and plain forms
static int32_t decrypt_sum_device(pvw_ctx* c, KeyRef key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D, const uint8_t* d_valid,
                                  const i64* d_weights, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                  uint32_t* d_count, uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(key.rc);
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  PVW_TRY(decrypt_sum_checks(!d_c1s || !d_c2col || !d_out, D, in_repr));
  return device_call(c, stream, [&](hipStream_t s) { return sum_capture_check(c, s, sum_dpart_need(c), 0); },
                     [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(sum_buffer(c, w, s));
    const SumView v = sum_view(c, w);
    PVW_TRY(ct_sum_enqueue(c, w, s, d_c1s, d_c2col, c->poly(), 1, D, d_valid, d_weights, v.c1, v.c2, d_count));
    return decrypt_sum_tail(c, w, s, key, in_repr, d_noisy, rep);
  });
}
int32_t pvw_decrypt_sum_plain_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                     const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                     uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus, uint32_t wide_words,
                                     uint64_t* d_wide, void* stream) {
  return decrypt_sum_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, d_valid, nullptr, in_repr, d_noisy, d_out, d_noise, d_status, d_count, plain_modulus,
                            wide_words, d_wide, stream);
}
int32_t pvw_decrypt_sum_device_sk_plain(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                        const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out,
                                        uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus,
                                        uint32_t wide_words, uint64_t* d_wide, void* stream) {
  return decrypt_sum_device(c, key_resident(c, key), d_c1s, d_c2col, D, d_valid, nullptr, in_repr, d_noisy, d_out, d_noise, d_status, d_count, plain_modulus,
                            wide_words, d_wide, stream);
}
int32_t pvw_decrypt_sum_checked_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                       const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out, uint64_t* d_noise,
                                       uint32_t* d_status, uint32_t* d_count, void* stream) {
  return decrypt_sum_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, d_valid, nullptr, in_repr, d_noisy, d_out, d_noise, d_status, d_count, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_sum_device_sk_checked(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                          const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_noisy, uint64_t* d_out,
                                          uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count, void* stream) {
  return decrypt_sum_device(c, key_resident(c, key), d_c1s, d_c2col, D, d_valid, nullptr, in_repr, d_noisy, d_out, d_noise, d_status, d_count, 0, 0, nullptr, stream);
}
int32_t pvw_decrypt_lincomb_plain_device(pvw_ctx* c, const int64_t* d_sk, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                         const uint8_t* d_valid, const int64_t* d_weights, uint32_t in_repr, uint64_t* d_noisy,
                                         uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                         uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  PVW_TRY(need_weights(d_weights));
  return decrypt_sum_device(c, key_coeffs(c, d_sk), d_c1s, d_c2col, D, d_valid, d_weights, in_repr, d_noisy, d_out, d_noise, d_status,
                            d_count, plain_modulus, wide_words, d_wide, stream);
}
int32_t pvw_decrypt_lincomb_device_sk_plain(pvw_ctx* c, const pvw_sk* key, const uint64_t* d_c1s, const uint64_t* d_c2col, size_t D,
                                            const uint8_t* d_valid, const int64_t* d_weights, uint32_t in_repr, uint64_t* d_noisy,
                                            uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                            uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  PVW_TRY(need_weights(d_weights));
  return decrypt_sum_device(c, key_resident(c, key), d_c1s, d_c2col, D, d_valid, d_weights, in_repr, d_noisy, d_out, d_noise, d_status,
                            d_count, plain_modulus, wide_words, d_wide, stream);
}
// host buffers
static int32_t decrypt_sum_hostbuf(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                                   const uint8_t* valid, const i64* weights, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                   uint32_t* status, uint32_t* count, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out_u64, noise, status, plain_modulus, wide_words, wide, &rep));
  PVW_TRY(decrypt_sum_checks(!sk || !c1s || !c2col || !out_u64, D, in_repr));
  const size_t nv = count_valid(valid, weights, D);
  if (nv == 0) return no_valid_dealer(D, weights);
  PVW_TRY(ensure_device(c));
  const size_t P = c->poly(), k = c->k, l = c->l, per = chunk_1gib((k + 1) * P * 8, nv);
  Scratch sc;
  const size_t r_sk = sc.add(k * l * 8), r_c1 = sc.add(per * k * P * 8), r_c2 = sc.add(per * P * 8), r_w = sc.add(weights ? per * 8 : 0);
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_TRY(sum_buffer(c, w, w->stream));
    const SumView v = sum_view(c, w);
    const Report dev = rep.packed_at(v.io, 1);                        // out | noise | status | wide: the key holder's
    i64* d_sk = sc.at<i64>(r_sk);
    sc.secret(w, r_sk, r_sk);
    ws_mark_secret(w, v.io, Report::packed_bytes(1, rep.ww));
    PVW_HIP(hipMemcpyAsync(d_sk, sk, k * l * 8, hipMemcpyHostToDevice, w->stream));
    PVW_TRY(ct_sum_staged(c, w, sc.at(r_c1), sc.at(r_c2), per, c1s, c2col, P, 1, D, valid, weights, sc.at<i64>(r_w), v.c1, v.c2));
    PVW_TRY(decrypt_sum_tail(c, w, w->stream, key_coeffs(c, d_sk), in_repr, nullptr, dev));
    return dev.copy_to(rep, 1, hipMemcpyDeviceToHost, w->stream);
  });
  if (rc == PVW_OK && count) *count = (uint32_t)nv;
  return rc;
}
int32_t pvw_decrypt_sum_plain(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D, const uint8_t* valid,
                              uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint32_t* count,
                              uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  return decrypt_sum_hostbuf(c, sk, c1s, c2col, D, valid, nullptr, in_repr, out_u64, noise, status, count, plain_modulus, wide_words, wide);
}
int32_t pvw_decrypt_lincomb_plain(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                                  const uint8_t* valid, const int64_t* weights, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                  uint32_t* status, uint32_t* count, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  PVW_TRY(need_weights(weights));
  return decrypt_sum_hostbuf(c, sk, c1s, c2col, D, valid, weights, in_repr, out_u64, noise, status, count, plain_modulus, wide_words, wide);
}
int32_t pvw_decrypt_sum_checked(pvw_ctx* c, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2col, size_t D,
                                const uint8_t* valid, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status,
                                uint32_t* count) {
  return pvw_decrypt_sum_plain(c, sk, c1s, c2col, D, valid, in_repr, out_u64, noise, status, count, 0, 0, nullptr);
}

// Every party's aggregate share: the sum over c1 and rows [lo, hi) of c2 (row r at its global position of the sum buffer, so the
// buffer reads as ONE whole ciphertext), then decrypt_all_run on that one ciphertext: the 22-party dispatch is its own.
static int32_t decrypt_all_sum_tail(pvw_ctx* c, Workspace* w, hipStream_t s, u32 lo, u32 hi, const int64_t* d_sk, uint32_t in_repr,
                                    const Report& rep) {
  const SumView v = sum_view(c, w);
  if (in_repr == PVW_REPR_POWER) {
    ProfScope ps(c, "ntt", s);
    PVW_HIP(launch_ntt(v.c1, c->k, false, c->dt, c->L, c->l, s));
    PVW_HIP(launch_ntt(v.c2 + (size_t)lo * c->poly(), hi - lo, false, c->dt, c->L, c->l, s));
  }
  return decrypt_all_run(c, w, s, AllCall{lo, (size_t)hi - lo, 1, d_sk, v.c1, v.c2, false, false, rep});
}
static int32_t decrypt_all_sum_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                      const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, const i64* d_weights, uint32_t in_repr,
                                      uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus,
                                      uint32_t wide_words, uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, d_sk, d_c1s, d_c2s, D, in_repr, d_out));
  PVW_TRY(check_dealers(D, true));
  const size_t P = c->poly(), need = decrypt_all_sum_need(c, (size_t)hi - lo, rep.ww);
  return device_call(c, stream, [&](hipStream_t s) { return sum_capture_check(c, s, sum_dpart_need(c), need); },
                     [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(sum_buffer(c, w, s));
    PVW_TRY(ws_scratch(w, need));                                    // before anything of this call is enqueued
    const SumView v = sum_view(c, w);
    PVW_TRY(ct_sum_enqueue(c, w, s, d_c1s, d_c2s + (size_t)lo * P, (size_t)c->n * P, hi - lo, D, d_valid, d_weights, v.c1,
                           v.c2 + (size_t)lo * P, d_count));
    return decrypt_all_sum_tail(c, w, s, lo, hi, d_sk, in_repr, rep);
  });
}
int32_t pvw_decrypt_all_sum_plain_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                         const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_out,
                                         uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus,
                                         uint32_t wide_words, uint64_t* d_wide, void* stream) {
  return decrypt_all_sum_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, d_valid, nullptr, in_repr, d_out, d_noise, d_status, d_count,
                                plain_modulus, wide_words, d_wide, stream);
}
int32_t pvw_decrypt_all_lincomb_plain_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                             const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, const int64_t* d_weights,
                                             uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count,
                                             uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide, void* stream) {
  PVW_TRY(need_weights(d_weights));
  return decrypt_all_sum_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, d_valid, d_weights, in_repr, d_out, d_noise, d_status, d_count,
                                plain_modulus, wide_words, d_wide, stream);
}
int32_t pvw_decrypt_all_sum_checked_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                           const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, uint32_t in_repr, uint64_t* d_out,
                                           uint64_t* d_noise, uint32_t* d_status, uint32_t* d_count, void* stream) {
  return pvw_decrypt_all_sum_plain_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, d_valid, in_repr, d_out, d_noise, d_status, d_count, 0, 0,
                                          nullptr, stream);
}
static int32_t decrypt_all_sum_hostbuf(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                       size_t D, const uint8_t* valid, const i64* weights, uint32_t in_repr, uint64_t* out_u64,
                                       uint64_t* noise, uint32_t* status, uint32_t* count, uint64_t plain_modulus, uint32_t wide_words,
                                       uint64_t* wide) {
  Report rep;
  PVW_TRY(report_args(c, out_u64, noise, status, plain_modulus, wide_words, wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, sk, c1s, c2s, D, in_repr, out_u64));
  PVW_TRY(check_dealers(D, true));
  const size_t nv = count_valid(valid, weights, D);
  if (nv == 0) return no_valid_dealer(D, weights);
  PVW_TRY(ensure_device(c));
  const size_t P = c->poly(), k = c->k, l = c->l, NP = (size_t)hi - lo, per = chunk_1gib((k + NP) * P * 8, nv);
  const size_t need = decrypt_all_sum_need(c, NP, rep.ww);
  // the staged pieces and the decrypt's own scratch share the front of the block (stream order: the sum has read the pieces
  // before the decrypt writes there); the uploaded keys sit behind both
  Scratch st;
  const size_t r_c1 = st.add(per * k * P * 8), r_c2 = st.add(per * NP * P * 8), r_w = st.add(weights ? per * 8 : 0);
  Scratch sc;
  const size_t r_main = sc.add(need > st.total ? need : st.total), r_sk = sc.add(NP * k * l * 8);
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_TRY(sum_buffer(c, w, w->stream));
    st.base = sc.at<char>(r_main);
    const SumView v = sum_view(c, w);
    const Report dev = rep.packed_at(v.io, c->n);
    i64* d_sk = sc.at<i64>(r_sk);
    sc.secret(w, r_sk, r_sk);
    ws_mark_secret(w, v.io, Report::packed_bytes(c->n, rep.ww));
    PVW_HIP(hipMemcpyAsync(d_sk, sk, NP * k * l * 8, hipMemcpyHostToDevice, w->stream));
    PVW_TRY(ct_sum_staged(c, w, st.at(r_c1), st.at(r_c2), per, c1s, c2s + (size_t)lo * P, (size_t)c->n * P, NP, D, valid, weights,
                          st.at<i64>(r_w), v.c1, v.c2 + (size_t)lo * P));
    PVW_TRY(decrypt_all_sum_tail(c, w, w->stream, lo, hi, d_sk, in_repr, dev));
    return dev.copy_to(rep, NP, hipMemcpyDeviceToHost, w->stream);
  });
  if (rc == PVW_OK && count) *count = (uint32_t)nv;
  return rc;
}
int32_t pvw_decrypt_all_sum_plain(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                  size_t D, const uint8_t* valid, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status,
                                  uint32_t* count, uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  return decrypt_all_sum_hostbuf(c, lo, hi, sk, c1s, c2s, D, valid, nullptr, in_repr, out_u64, noise, status, count, plain_modulus,
                                 wide_words, wide);
}
int32_t pvw_decrypt_all_lincomb_plain(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                      size_t D, const uint8_t* valid, const int64_t* weights, uint32_t in_repr, uint64_t* out_u64,
                                      uint64_t* noise, uint32_t* status, uint32_t* count, uint64_t plain_modulus, uint32_t wide_words,
                                      uint64_t* wide) {
  PVW_TRY(need_weights(weights));
  return decrypt_all_sum_hostbuf(c, lo, hi, sk, c1s, c2s, D, valid, weights, in_repr, out_u64, noise, status, count, plain_modulus,
                                 wide_words, wide);
}
int32_t pvw_decrypt_all_sum_checked(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                    size_t D, const uint8_t* valid, uint32_t in_repr, uint64_t* out_u64, uint64_t* noise,
                                    uint32_t* status, uint32_t* count) {
  return pvw_decrypt_all_sum_plain(c, lo, hi, sk, c1s, c2s, D, valid, in_repr, out_u64, noise, status, count, 0, 0, nullptr);
}

// Every party's share of R combinations.  The sum buffer holds one combined ciphertext, so the R of them (public)
// go into the stream's scratch as whole ciphertexts, c1 [R][k] | c2 [R][n] (row j at its global position), a POWER-basis input is
// transformed there, and ONE decrypt_all_run with the combinations in the dealers' place follows: its 22-party dispatch, GEMM
// path, plain decode and hygiene are its own.  R is cut into groups of at most one staging budget of combined ciphertexts; each
// group is one more set of passes over the dealers and fills its block of columns of the [P][R] report.
struct ManyLayout {
  size_t Rg, need;                    // combinations per group; the decrypt's own scratch (the front of the block)
  Scratch sc;
  size_t r_main, r_cc1, r_cc2;
};
static ManyLayout decrypt_all_many_layout(const pvw_ctx* c, size_t NP, size_t R, size_t ww, size_t front) {
  const size_t P = c->poly();
  ManyLayout m;
  m.Rg = chunk_1gib(((size_t)c->k + c->n) * P * 8, R);
  m.need = decrypt_all_layout(c, NP, m.Rg, false, false, true, true, ww).sc.total;
  if (R % m.Rg) {                                                  // the last group's own layout (not monotone in the count)
    const size_t last = decrypt_all_layout(c, NP, R % m.Rg, false, false, true, true, ww).sc.total;
    if (last > m.need) m.need = last;
  }
  m.r_main = m.sc.add(m.need > front ? m.need : front);
  m.r_cc1 = m.sc.add(m.Rg * c->k * P * 8), m.r_cc2 = m.sc.add(m.Rg * c->n * P * 8);
  return m;
}
// the group's combined ciphertexts are in place: transform (POWER basis) and decrypt into columns [r0, r0 + cnt) of rep [P][R]
static int32_t decrypt_all_many_tail(pvw_ctx* c, Workspace* w, hipStream_t s, u32 lo, u32 hi, const int64_t* d_sk, uint32_t in_repr,
                                     u64* cc1, u64* cc2, size_t cnt, const Report& rep, size_t ld) {
  const size_t P = c->poly();
  if (in_repr == PVW_REPR_POWER) {
    ProfScope ps(c, "ntt", s);
    PVW_HIP(launch_ntt(cc1, cnt * c->k, false, c->dt, c->L, c->l, s));
    for (size_t r = 0; r < cnt; ++r) PVW_HIP(launch_ntt(cc2 + (r * c->n + lo) * P, hi - lo, false, c->dt, c->L, c->l, s));
  }
  AllCall q{lo, (size_t)hi - lo, cnt, d_sk, cc1, cc2, false, false, rep};
  q.rep_ld = ld;
  return decrypt_all_run(c, w, s, q);
}
int32_t pvw_decrypt_all_lincomb_many_plain_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                                  const uint64_t* d_c2s, size_t D, const uint8_t* d_valid, const int64_t* d_weights,
                                                  size_t R, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise, uint32_t* d_status,
                                                  uint32_t* d_counts, uint64_t plain_modulus, uint32_t wide_words, uint64_t* d_wide,
                                                  void* stream) {
  PVW_TRY(need_weights(d_weights));
  if (R == 1)
    return decrypt_all_sum_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, d_valid, d_weights, in_repr, d_out, d_noise, d_status, d_counts,
                                  plain_modulus, wide_words, d_wide, stream);
  Report rep;
  PVW_TRY(report_args(c, d_out, d_noise, d_status, plain_modulus, wide_words, d_wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, d_sk, d_c1s, d_c2s, D, in_repr, d_out));
  PVW_TRY(check_dealers(D, true));
  PVW_TRY(combos_check(R, true));
  const size_t P = c->poly(), NP = (size_t)hi - lo;
  ManyLayout m = decrypt_all_many_layout(c, NP, R, rep.ww, 0);
  // as the checked reconstruction: the caller's stream is looked at before the device is initialised
  auto sized = [&](hipStream_t s) -> int32_t {
    PVW_TRY(grown_capture_check(c, s, &Workspace::scratch_bytes, m.sc.total,
                                "many combinations under stream capture: run a call with the same party range and at least as many "
                                "combinations on this stream outside capture first (it sizes the scratch)"));
    return sum_capture_check(c, s, 0, 0);
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  return device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(sum_buffer(c, w, s));
    PVW_TRY(m.sc.take(w));                                           // before anything of this call is enqueued
    u64 *cc1 = m.sc.at(m.r_cc1), *cc2 = m.sc.at(m.r_cc2);
    for (size_t r0 = 0; r0 < R; r0 += m.Rg) {
      const size_t cnt = (R - r0) < m.Rg ? (R - r0) : m.Rg;
      u32* cnts = d_counts ? d_counts + r0 : nullptr;
      PVW_TRY(ct_sum_enqueue(c, w, s, d_c1s, d_c2s + (size_t)lo * P, (size_t)c->n * P, NP, D, d_valid, d_weights + r0 * D, cc1,
                             cc2 + (size_t)lo * P, cnts, false, Combos{cnt, D, (size_t)c->k * P, (size_t)c->n * P}));
      PVW_TRY(decrypt_all_many_tail(c, w, s, lo, hi, d_sk, in_repr, cc1, cc2, cnt, rep.at(r0), R));
    }
    return PVW_OK;
  });
}
int32_t pvw_decrypt_all_lincomb_many_plain(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s,
                                           const uint64_t* c2s, size_t D, const uint8_t* valid, const int64_t* weights, size_t R,
                                           uint32_t in_repr, uint64_t* out_u64, uint64_t* noise, uint32_t* status, uint32_t* counts,
                                           uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  PVW_TRY(need_weights(weights));
  if (R == 1)
    return decrypt_all_sum_hostbuf(c, lo, hi, sk, c1s, c2s, D, valid, weights, in_repr, out_u64, noise, status, counts, plain_modulus,
                                   wide_words, wide);
  Report rep;
  PVW_TRY(report_args(c, out_u64, noise, status, plain_modulus, wide_words, wide, &rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, sk, c1s, c2s, D, in_repr, out_u64));
  PVW_TRY(check_dealers(D, true));
  PVW_TRY(combos_check(R, false));
  const size_t nv = count_valid_any(valid, weights, D, R);
  if (nv == 0) return no_valid_dealer(D, weights);
  PVW_TRY(ensure_device(c));
  const size_t P = c->poly(), k = c->k, l = c->l, NP = (size_t)hi - lo, per = chunk_1gib((k + NP) * P * 8, nv);
  // the staged pieces and the decrypt's own scratch share the front of the block, as in decrypt_all_sum_hostbuf; behind them the
  // combined ciphertexts, the group's report [P][Rg] and the uploaded keys
  Scratch st;
  const size_t r_c1 = st.add(per * k * P * 8), r_c2 = st.add(per * NP * P * 8);
  ManyLayout m = decrypt_all_many_layout(c, NP, R, rep.ww, 0);
  const size_t r_w = st.add(m.Rg * per * 8);
  m = decrypt_all_many_layout(c, NP, R, rep.ww, st.total);
  const size_t r_io = m.sc.add(Report::packed_bytes(NP * m.Rg, rep.ww)), r_sk = m.sc.add(NP * k * l * 8);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(m.sc.take(w));
    PVW_TRY(sum_buffer(c, w, w->stream));
    st.base = m.sc.at<char>(m.r_main);
    u64 *cc1 = m.sc.at(m.r_cc1), *cc2 = m.sc.at(m.r_cc2);
    i64* d_sk = m.sc.at<i64>(r_sk);
    m.sc.secret(w, r_io, r_sk);
    PVW_HIP(hipMemcpyAsync(d_sk, sk, NP * k * l * 8, hipMemcpyHostToDevice, w->stream));
    for (size_t r0 = 0; r0 < R; r0 += m.Rg) {
      const size_t cnt = (R - r0) < m.Rg ? (R - r0) : m.Rg;
      const i64* wr = weights + r0 * D;
      if (count_valid_any(valid, wr, D, cnt) == 0) {                  // nobody takes part in this group's rows: zeros
        PVW_HIP(hipMemsetAsync(cc1, 0, cnt * k * P * 8, w->stream));
        PVW_HIP(hipMemsetAsync(cc2, 0, cnt * c->n * P * 8, w->stream));
      } else {
        PVW_TRY(ct_sum_staged(c, w, st.at(r_c1), st.at(r_c2), per, c1s, c2s + (size_t)lo * P, (size_t)c->n * P, NP, D, valid, wr,
                              st.at<i64>(r_w), cc1, cc2 + (size_t)lo * P, cnt, k * P, (size_t)c->n * P));
      }
      const Report dev = rep.packed_at(m.sc.at(r_io), NP * cnt);
      PVW_TRY(decrypt_all_many_tail(c, w, w->stream, lo, hi, d_sk, in_repr, cc1, cc2, cnt, dev, 0));
      PVW_TRY(dev.copy_block_to(rep.at(r0), NP, cnt, R, hipMemcpyDeviceToHost, w->stream));
      combo_counts(valid, wr, D, cnt, counts ? counts + r0 : nullptr);
    }
    return PVW_OK;
  });
}

// Advisory: for how many dealers at the builder's noise bound the gadget decode of the aggregate is PROVEN exact.  With
// z_j = -P Delta^j + n_j and max |n_j| <= R, R (Delta^(l-1) + 1) < Q / 2, every tmp_i and the Horner value
// n_0 Delta^(l-1) - n_(l-1) of decryption.rs:10-58 stay below Q / 2 in magnitude, so the chain is exact: sufficient, not
// necessary.  Q is odd: R = floor((Q - 1) / (2 (Delta^(l-1) + 1))).
int32_t pvw_ctx_sum_capacity(const pvw_ctx* c, uint64_t* max_dealers) {
  if (!c || !max_dealers) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  uint64_t nb = 0;
  PVW_TRY(pvw_ctx_noise_bound(c, &nb));
  const BigInt R = (c->Q - BigInt(1)) / ((c->delta_pow + BigInt(1)) * BigInt(2));
  const BigInt cap = nb ? R / BigInt(nb) : R;
  *max_dealers = cap.fits_u64() ? (cap.mag.empty() ? 0 : cap.mag[0]) : ~(uint64_t)0;
  return PVW_OK;
}
// Advisory, the weighted form of the same radius: *fits = 1 iff (sum over the participating dealers of |w_d|) noise_bound <= R.
// A weight multiplies its dealer's noise by |w|, so this is the sufficient condition of pvw_ctx_sum_capacity with the dealer
// count replaced by the weights' absolute sum.  Host big integers (|INT64_MIN| = 2^63 is no special case there).
int32_t pvw_ctx_lincomb_fits(const pvw_ctx* c, const int64_t* weights, size_t D, const uint8_t* valid, uint32_t* fits) {
  if (!c || !weights || !fits) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  uint64_t nb = 0;
  PVW_TRY(pvw_ctx_noise_bound(c, &nb));
  const BigInt R = (c->Q - BigInt(1)) / ((c->delta_pow + BigInt(1)) * BigInt(2));
  BigInt sum;
  for (size_t d = 0; d < D; ++d)
    if (takes_part(valid, weights, d)) sum = sum + BigInt(weights[d] < 0 ? (u64)0 - (u64)weights[d] : (u64)weights[d]);
  *fits = sum * BigInt(nb) <= R ? 1u : 0u;
  return PVW_OK;
}
// the words a digit plaintext of the wide handover takes: |P_v| < num_valid NL 2^(b - 1) 2^limb_bits
static u32 handover_wide_words(size_t num_valid, u32 NL, u32 limb_bits, u32 digit_bits) {
  const u64 terms = (u64)num_valid * NL;
  u32 lg = 0;
  while (lg < 64 && ((u64)1 << lg) < terms) ++lg;                  // ceil(log2(terms))
  return (limb_bits + digit_bits + lg + 1 + 63) / 64;
}
// Advisory, pvw_ctx_lincomb_fits for the rows of a wide handover without the rows: every weight is a signed digit of digit_bits
// bits, so num_valid NL 2^(digit_bits - 1) bounds a row's absolute sum; and the digit plaintexts must fit the words of Q.
int32_t pvw_ctx_wide_handover_fits(const pvw_ctx* c, const uint64_t* plain_modulus, size_t num_valid, uint32_t limb_bits,
                                   uint32_t digit_bits, uint32_t* fits) {
  if (!c || !plain_modulus || !fits) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (num_valid == 0) return fail(PVW_ERR_INVALID_PARAMETERS, "no valid holder");
  WideMod m;
  PVW_TRY(wide_modulus_check(plain_modulus, &m));
  uint32_t NL = 0;
  PVW_TRY(wide_limb_count(m, limb_bits, &NL));
  PVW_TRY(digit_bits_check(digit_bits));
  uint64_t nb = 0;
  PVW_TRY(pvw_ctx_noise_bound(c, &nb));
  const BigInt R = (c->Q - BigInt(1)) / ((c->delta_pow + BigInt(1)) * BigInt(2));
  const BigInt sum = BigInt((u64)num_valid) * BigInt((u64)NL) * BigInt((u64)1 << (digit_bits - 1));
  *fits = (sum * BigInt(nb) <= R && handover_wide_words(num_valid, NL, limb_bits, digit_bits) <= c->Q.mag.size()) ? 1u : 0u;
  return PVW_OK;
}

// Every new party's new share from the old holders' limb ciphertexts in one call: the weight rows by the kernels
// of pvw_shamir_wide_handover_weights_device, the many-combinations call of 8.15 as it is with R = T V rows over the D NL
// vectors and wide_words = ww, and the fold of pvw_shamir_wide_from_digits_device over its report, read in place.  The weights
// and the combined ciphertexts are public; the report [P][R] (values, words, status) depends on the shares: it is marked secret
// and cleared behind the fold.  The keys are staged, marked and cleared by the many-combinations call itself.
struct HandoverIo {
  size_t NP, R, ww, ld;
  size_t b_w, b_res, b_wide, b_st;
  HandoverIo(size_t NP_, const HandoverWide& h, size_t ww_) : NP(NP_), R(h.rows()), ww(ww_), ld(h.ld()) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    b_w = up(R * ld * 8), b_res = up(NP * R * 8), b_wide = up(NP * R * ww * 8), b_st = up(NP * R * 4);
  }
  size_t report_bytes() const { return b_res + b_wide + b_st; }
  size_t total() const { return b_w + report_bytes(); }
  i64* weights(char* base) const { return (i64*)base; }
  u64* res(char* base) const { return (u64*)(base + b_w); }
  u64* wide(char* base) const { return (u64*)(base + b_w + b_res); }
  u32* status(char* base) const { return (u32*)(base + b_w + b_res + b_wide); }
};
// the order: NULL, the checks of the weights, the words of Q, then what the many-combinations call refuses about its arguments
static int32_t handover_all_checks(pvw_ctx* c, u32 lo, u32 hi, const void* sk, const void* c1s, const void* c2s, HandoverWide& h,
                                   uint32_t in_repr, const void* out, const void* status, bool device, u32* ww) {
  if (!c || !out || !status) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(handover_wide_checks(h, out, device));
  *ww = handover_wide_words(h.nv(), h.NL, h.limb_bits, h.digit_bits);
  if (*ww > c->Q.mag.size()) {
    char buf[128];
    snprintf(buf, sizeof buf, "the digit plaintexts of this handover take %u words, Q has %zu: choose narrower digits", *ww, c->Q.mag.size());
    return fail(PVW_ERR_INVALID_PARAMETERS, buf);
  }
  PVW_TRY(decrypt_all_checks(c, lo, hi, sk, c1s, c2s, h.ld(), in_repr, out));
  PVW_TRY(check_dealers(h.ld(), true));
  return combos_check(h.rows(), device);
}
static const char* const kHandoverUnsized =
    "wide handover under stream capture: run a call with the same party range, at least as many valid holders, target points and "
    "vectors on this stream outside capture first (it sizes the scratch)";
// what pvw_decrypt_all_lincomb_many_plain_device asks of a capturing stream, asked before anything of the handover is enqueued
static int32_t handover_many_capture_check(pvw_ctx* c, hipStream_t s, size_t NP, size_t R, size_t ww, const char* msg = kHandoverUnsized) {
  if (R == 1) return sum_capture_check(c, s, sum_dpart_need(c), decrypt_all_sum_need(c, NP, ww));
  const ManyLayout m = decrypt_all_many_layout(c, NP, R, ww, 0);
  PVW_TRY(grown_capture_check(c, s, &Workspace::scratch_bytes, m.sc.total, msg));
  return sum_capture_check(c, s, 0, 0);
}
int32_t pvw_decrypt_all_handover_wide_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                             const uint64_t* d_c2s, size_t num_dealers, const uint64_t* plain_modulus, uint32_t limb_bits,
                                             uint32_t digit_bits, const uint64_t* indices, const uint8_t* valid, const uint64_t* points,
                                             size_t num_points, uint32_t in_repr, uint64_t* d_out, uint32_t* d_status, uint32_t* d_count,
                                             void* stream) {
  HandoverWide h{plain_modulus, indices, valid, num_dealers, points, num_points, limb_bits, digit_bits};
  u32 ww = 0;
  PVW_TRY(handover_all_checks(c, lo, hi, d_sk, d_c1s, d_c2s, h, in_repr, d_out, d_status, true, &ww));
  const size_t NP = (size_t)hi - lo;
  const HandoverIo io(NP, h, ww);
  const size_t pub_need = handover_wide_ws_bytes(h);
  auto sized = [&](hipStream_t s) -> int32_t {
    PVW_TRY(grown_capture_check(c, s, &Workspace::handover_wide_bytes, pub_need, kHandoverUnsized));
    PVW_TRY(grown_capture_check(c, s, &Workspace::handover_io_bytes, io.total(), kHandoverUnsized));
    return handover_many_capture_check(c, s, NP, io.R, ww);
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  char* base = nullptr;
  PVW_TRY(device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(ws_grow(&w->handover_wide, &w->handover_wide_bytes, pub_need, s, false));
    if (w->handover_io_bytes < io.total()) ws_public(w, w->handover_io, w->handover_io_bytes);   // the block is about to go
    PVW_TRY(ws_grow(&w->handover_io, &w->handover_io_bytes, io.total(), s, true));
    base = (char*)w->handover_io;
    return handover_wide_weights_enqueue(c, h, w->handover_wide, io.weights(base), s);
  }));
  const int32_t rc = pvw_decrypt_all_lincomb_many_plain_device(c, lo, hi, d_sk, d_c1s, d_c2s, io.ld, nullptr, io.weights(base), io.R, in_repr,
                                                               io.res(base), nullptr, io.status(base), nullptr, 0, ww, io.wide(base), stream);
  const WideMont mm = make_wide_mont(plain_modulus);
  return device_call(c, stream, [&](Workspace* w, hipStream_t s) -> int32_t {
    ws_mark_secret(w, io.res(base), io.report_bytes());              // cleared by device_end, also behind a pass that failed
    if (rc != PVW_OK) return rc;
    ProfScope ps(c, "shamir_wide_from_digits", s);
    PVW_HIP(launch_shamir_wide_from_digits(io.wide(base), io.status(base), NP * h.T, h.V, ww, h.digit_bits, d_out, d_status, h.m, mm, s));
    const u32 nv = (u32)h.nv();
    if (d_count) PVW_HIP(launch_shamir_handover_columns(&nv, 1, d_count, s));
    return PVW_OK;
  });
}
// host buffers: the weights by the same kernels on a pooled workspace, the many-combinations call on host buffers (its staging
// in pieces, its key hygiene), the fold by its kernel on a pooled workspace; the host copies of the report are wiped
int32_t pvw_decrypt_all_handover_wide(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                      size_t num_dealers, const uint64_t* plain_modulus, uint32_t limb_bits, uint32_t digit_bits,
                                      const uint64_t* indices, const uint8_t* valid, const uint64_t* points, size_t num_points,
                                      uint32_t in_repr, uint64_t* out, uint32_t* status, uint32_t* count) {
  HandoverWide h{plain_modulus, indices, valid, num_dealers, points, num_points, limb_bits, digit_bits};
  u32 ww = 0;
  PVW_TRY(handover_all_checks(c, lo, hi, sk, c1s, c2s, h, in_repr, out, status, false, &ww));
  PVW_TRY(ensure_device(c));
  const size_t NP = (size_t)hi - lo, R = h.rows(), ld = h.ld(), cnt = NP * h.T;
  std::vector<i64> wts(R * ld);
  {
    Scratch sc;
    const size_t r_pub = sc.add(handover_wide_ws_bytes(h)), r_w = sc.add(R * ld * 8);
    PVW_TRY(host_call(c, [&](Workspace* w) -> int32_t {
      PVW_TRY(sc.take(w));
      PVW_TRY(handover_wide_weights_enqueue(c, h, sc.at(r_pub), sc.at<i64>(r_w), w->stream));
      PVW_HIP(hipMemcpyAsync(wts.data(), sc.at(r_w), R * ld * 8, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    }));
  }
  std::vector<u64> res(NP * R), wide(NP * R * ww);
  std::vector<u32> st(NP * R);
  int32_t rc = pvw_decrypt_all_lincomb_many_plain(c, lo, hi, sk, c1s, c2s, ld, nullptr, wts.data(), R, in_repr, res.data(), nullptr, st.data(),
                                                  nullptr, 0, ww, wide.data());
  if (rc == PVW_OK) {
    const WideMont mm = make_wide_mont(plain_modulus);
    Scratch sc;
    const size_t r_wide = sc.add(wide.size() * 8), r_st = sc.add(st.size() * 4), r_out = sc.add(cnt * 32), r_so = sc.add(cnt * 4);
    rc = host_call(c, [&](Workspace* w) -> int32_t {
      PVW_TRY(sc.take(w));
      sc.secret(w, r_wide, r_so);
      PVW_HIP(hipMemcpyAsync(sc.at(r_wide), wide.data(), wide.size() * 8, hipMemcpyHostToDevice, w->stream));
      PVW_HIP(hipMemcpyAsync(sc.at(r_st), st.data(), st.size() * 4, hipMemcpyHostToDevice, w->stream));
      ProfScope ps(c, "shamir_wide_from_digits", w->stream);
      PVW_HIP(launch_shamir_wide_from_digits(sc.at(r_wide), sc.at<u32>(r_st), cnt, h.V, ww, h.digit_bits, sc.at(r_out), sc.at<u32>(r_so), h.m, mm,
                                             w->stream));
      PVW_HIP(hipMemcpyAsync(out, sc.at(r_out), cnt * 32, hipMemcpyDeviceToHost, w->stream));
      PVW_HIP(hipMemcpyAsync(status, sc.at(r_so), cnt * 4, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    });
  }
  volatile u64* vp = wide.data();
  for (size_t i = 0; i < wide.size(); ++i) vp[i] = 0;
  vp = res.data();
  for (size_t i = 0; i < res.size(); ++i) vp[i] = 0;
  if (rc == PVW_OK && count) *count = (uint32_t)h.nv();
  return rc;
}

// The one-word handover in one call: the weight rows by the kernels of pvw_shamir_handover_weights_device from a
// mask read when they run, then the many-combinations call of 8.15 ITSELF with R = T rows and valid = NULL -- a masked holder's
// weights are 0, so its ciphertext is never addressed -- and that call's report as it is.  The rows are public; keys and report
// are the many-combinations call's to stage, mark and clear.
// the order: NULL, the checks of the weights, the report's arguments, then what the many-combinations call refuses
static int32_t handover_narrow_checks(pvw_ctx* c, u32 lo, u32 hi, const void* sk, const void* c1s, const void* c2s, size_t D,
                                      const u64* indices, const u64* targets, size_t T, uint32_t in_repr, u64* out, u64* noise, u32* status,
                                      u64 p, u32 wide_words, u64* wide, bool device, Report* rep) {
  if (!c || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(handover_checks(p, indices, D, targets, T, out, device));
  PVW_TRY(report_args(c, out, noise, status, p, wide_words, wide, rep));
  PVW_TRY(decrypt_all_checks(c, lo, hi, sk, c1s, c2s, D, in_repr, out));
  PVW_TRY(check_dealers(D, true));
  return combos_check(T, device);
}
static const char* const kHandoverNarrowUnsized =
    "handover under stream capture: run a call with the same party range and at least as many holders and target points on this "
    "stream outside capture first (it sizes the workspace and the scratch)";
int32_t pvw_decrypt_all_handover_device(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* d_sk, const uint64_t* d_c1s,
                                        const uint64_t* d_c2s, size_t num_holders, const uint8_t* d_valid, const uint64_t* indices,
                                        const uint64_t* targets, size_t num_targets, uint32_t in_repr, uint64_t* d_out, uint64_t* d_noise,
                                        uint32_t* d_status, uint32_t* d_count, uint64_t plain_modulus, uint32_t wide_words,
                                        uint64_t* d_wide, void* stream) {
  Report rep;
  PVW_TRY(handover_narrow_checks(c, lo, hi, d_sk, d_c1s, d_c2s, num_holders, indices, targets, num_targets, in_repr, d_out, d_noise, d_status,
                                 plain_modulus, wide_words, d_wide, true, &rep));
  const size_t NP = (size_t)hi - lo, D = num_holders, T = num_targets;
  const size_t pub_need = handover_ws_bytes(D, T), rows_need = T * D * 8;
  auto sized = [&](hipStream_t s) -> int32_t {
    PVW_TRY(grown_capture_check(c, s, &Workspace::handover_bytes, pub_need, kHandoverNarrowUnsized));
    PVW_TRY(grown_capture_check(c, s, &Workspace::handover_rows_bytes, rows_need, kHandoverNarrowUnsized));
    return handover_many_capture_check(c, s, NP, T, rep.ww, kHandoverNarrowUnsized);
  };
  if (stream) PVW_TRY(sized((hipStream_t)stream));
  i64* rows = nullptr;
  PVW_TRY(device_call(c, stream, sized, [&](Workspace* w, hipStream_t s) -> int32_t {
    PVW_TRY(ws_grow(&w->handover, &w->handover_bytes, pub_need, s, false));          // public: nothing to clear
    PVW_TRY(ws_grow(&w->handover_rows, &w->handover_rows_bytes, rows_need, s, false));
    rows = (i64*)w->handover_rows;
    return handover_weights_enqueue(c, plain_modulus, indices, d_valid, D, targets, T, w->handover, rows, d_count, s);
  }));
  return pvw_decrypt_all_lincomb_many_plain_device(c, lo, hi, d_sk, d_c1s, d_c2s, D, nullptr, rows, T, in_repr, d_out, d_noise, d_status,
                                                   nullptr, plain_modulus, wide_words, d_wide, stream);
}
// host buffers: the weights by the same kernels on a pooled workspace (the mask goes up with the call), then the many-combinations
// call on host buffers with the caller's mask: its staging of the valid holders in pieces, its key hygiene, its refusals
int32_t pvw_decrypt_all_handover(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const uint64_t* c1s, const uint64_t* c2s,
                                 size_t num_holders, const uint8_t* valid, const uint64_t* indices, const uint64_t* targets,
                                 size_t num_targets, uint32_t in_repr, uint64_t* out, uint64_t* noise, uint32_t* status, uint32_t* count,
                                 uint64_t plain_modulus, uint32_t wide_words, uint64_t* wide) {
  Report rep;
  PVW_TRY(handover_narrow_checks(c, lo, hi, sk, c1s, c2s, num_holders, indices, targets, num_targets, in_repr, out, noise, status,
                                 plain_modulus, wide_words, wide, false, &rep));
  const size_t D = num_holders, T = num_targets;
  size_t nv = 0;
  for (size_t d = 0; d < D; ++d) nv += !valid || valid[d];
  if (nv == 0) return no_valid_dealer(D, nullptr);
  PVW_TRY(ensure_device(c));
  std::vector<i64> wts(T * D);
  {
    Scratch sc;
    const size_t r_pub = sc.add(handover_ws_bytes(D, T)), r_w = sc.add(T * D * 8), r_v = sc.add(D);
    PVW_TRY(host_call(c, [&](Workspace* w) -> int32_t {
      PVW_TRY(sc.take(w));
      uint8_t* d_valid = valid ? sc.at<uint8_t>(r_v) : nullptr;
      if (valid) PVW_HIP(hipMemcpyAsync(d_valid, valid, D, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(handover_weights_enqueue(c, plain_modulus, indices, d_valid, D, targets, T, sc.at(r_pub), sc.at<i64>(r_w), nullptr, w->stream));
      PVW_HIP(hipMemcpyAsync(wts.data(), sc.at(r_w), T * D * 8, hipMemcpyDeviceToHost, w->stream));
      return PVW_OK;
    }));
  }
  const int32_t rc = pvw_decrypt_all_lincomb_many_plain(c, lo, hi, sk, c1s, c2s, D, valid, wts.data(), T, in_repr, out, noise, status, nullptr,
                                                        plain_modulus, wide_words, wide);
  if (rc == PVW_OK && count) *count = (uint32_t)nv;
  return rc;
}

// ------------------------------------------------------------------------ key generation
// Where key generation gets the parties' secret keys: host coefficients [hi - lo][k][l] (pvw_keygen), or the seed they are
// drawn from on the device, by the kernel that transforms them (pvw_keygen_seeded; SecretKey::random, secret_key.rs:45-63:
// polynomial j of party p is the CBD stream (seed, DOM_SK, p * k + j)).  Exactly one is set.
struct KeySource {
  const int64_t* sk = nullptr;
  const uint8_t* sk_seed = nullptr;
  bool seeded() const { return sk_seed != nullptr; }
  // the `js` job of a key-generation prologue for the parties from p0 on: the uploaded coefficients at `coeffs`, or the
  // sampled family with its key beside the error key in pb.key[]
  int32_t job(const pvw_ctx* c, PrologueBatch& pb, PrologueJob& js, const i64* coeffs, u32 p0) const {
    js.sj.count = c->k;
    if (!seeded()) {
      js.explicit_coeffs = coeffs;
      js.rep_coeffs = (size_t)c->k * c->l;
      return PVW_OK;
    }
    PVW_TRY(cbd_job(c->variance, js.sj));
    js.sj.domain = DOM_SK; js.sj.index0 = p0 * c->k; js.rep_index0 = c->k;
    js.key_idx = 1;
    pb.key[1] = make_key(sk_seed);
    return PVW_OK;
  }
};

// b_i = s_i * A + e_i: for every party the k-term inner products over A's COLUMNS, i.e. one
// mac_rows pass over the transposed CRS per party (public_key.rs:111-147, crs.rs:138-171).
// The CRS is transposed once per call into a temporary tiled matrix; groups of 4 parties then
// share one pass over it (mac_rows_multi with s-hat_i in the role of r-hat).
// key generation on the matrix cores with the roles chosen so that the SHARED operand is digitised once:
//   b_p[col] = sum_j s-hat_p[j] * A-hat[j][col] + e_p[col]
// GEMM rows = parties (their s-hat rows are the raw streamed operand, MFMA-tiled per chunk), GEMM vectors = the k
// columns of A-hat (digit tiles built ONCE per call, straight from the CRS in API layout: no transpose), the
// finish pass adds e_p and writes into the tiled B-hat.  Chunks of up to 1024 parties.
static int32_t keygen_gemm_swapped(pvw_ctx* c, Workspace* w, u32 a, u32 b, u32 lo, const KeySource& ks, const int64_t* ek,
                                   const uint8_t* seed) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly();
  hipStream_t s = w->stream;
  const u32 chunk = (b - a) < 1024 ? (b - a) : 1024;
  const u32 nb = (k + 15) / 16;                                      // batches of 16 column-vectors
  const bool direct = l <= 32;                                        // see the chunk loop
  Scratch sc;
  const size_t r_api = sc.add((size_t)k * k * P * 8);
  const size_t r_yd = sc.add(yd_bytes(16 * nb, k, L, l)), r_sy = sc.add(sy_bytes(16 * nb, L, l));   // whole batches: the last one is read in full
  const size_t small_bytes = ks.seeded() ? 0 : (size_t)2 * chunk * k * l * 8;   // seeded: nothing is uploaded
  const size_t r_small0 = sc.add(small_bytes), r_small1 = sc.add(small_bytes);   // sk | ek of one chunk, double buffered
  const size_t r_srow = sc.add(direct ? 0 : (size_t)chunk * k * P * 8);   // l = 64 only: s-hat rows | e rows, API layout [p][j or col][P]
  const size_t r_erow = sc.add(direct ? 0 : (size_t)chunk * k * P * 8);
  const size_t r_xm = sc.add(xm_words(chunk, k, L, l) * 8);
  const size_t r_tmp = sc.add((size_t)nb * gemm_tmp_words(chunk, L, l) * 8);
  PVW_TRY(sc.take(w));
  u64 *d_api = sc.at(r_api), *d_srow = sc.at(r_srow), *d_erow = sc.at(r_erow), *d_xm = sc.at(r_xm), *d_tmp = sc.at(r_tmp);
  signed char* d_yd = sc.at<signed char>(r_yd);
  int* d_sy = sc.at<int>(r_sy);
  i64* d_small2[2] = {sc.at<i64>(r_small0), sc.at<i64>(r_small1)};
  // everything derived from the secret keys: their coefficients (and explicit key errors), the MFMA-tiled copy of
  // NTT(s), the GEMM intermediate (s A without the error) and, for l = 64, the rows of NTT(s) and of the transformed
  // errors -- cleared when the call ends
  sc.secret(w, r_small0, r_tmp);
  // the secret keys of chunk i+1 are uploaded on a helper stream while chunk i computes
  const u32 nchunks = (b - a + chunk - 1) / chunk;
  const i64* sk = ks.sk;
  ShatDraw draw{};
  if (ks.seeded()) {                                                  // drawn keys: no buffers, helper stream or events
    SampleJob sj{};
    PVW_TRY(cbd_job(c->variance, sj));
    draw.key = make_key(ks.sk_seed); draw.cbd_half = sj.cbd_half; draw.cbd_v = sj.cbd_v;
  } else {
    PVW_TRY(ws_aux(w, 2 * (size_t)nchunks + 2));
  }
  auto upload = [&](u32 ci, hipStream_t st) -> int32_t {
    const u32 q0 = a + ci * chunk, cn = (b - q0) < chunk ? (b - q0) : chunk;
    const size_t wd = (size_t)cn * k * l;
    i64* dst = d_small2[ci & 1];
    PVW_HIP(hipMemcpyAsync(dst, sk + (size_t)(q0 - lo) * k * l, wd * 8, hipMemcpyHostToDevice, st));
    if (ek) PVW_HIP(hipMemcpyAsync(dst + (size_t)chunk * k * l, ek + (size_t)(q0 - lo) * k * l, wd * 8, hipMemcpyHostToDevice, st));
    return PVW_OK;
  };
  if (!ks.seeded()) PVW_TRY(upload(0, s));
  // A-hat -> API layout [j][col][limb][slot]; vector `col` is its column: element j at col * P + limb * l + j * (k * P)
  PVW_HIP(launch_untile(c->dA, d_api, k, 0, k, L, l, false, c->dt, s));
  PVW_HIP(launch_vec_digits(d_api, P, d_yd, d_sy, k, k, L, l, c->dt, s, l, (size_t)k * P));
  for (u32 ci = 0; ci < nchunks; ++ci) {
    const u32 p0 = a + ci * chunk;
    const u32 cnt = (b - p0) < chunk ? (b - p0) : chunk;
    i64* d_small = d_small2[ci & 1];
    if (ci > 0 && !ks.seeded()) PVW_HIP(hipStreamWaitEvent(s, w->events[2 * ci], 0));          // this chunk's keys have arrived
    ProfScope ps(c, "keygen", s);
    // l <= 32: s-hat_p (secret_key.rs:98-112) goes straight from the uploaded coefficients into the MFMA-tiled raw
    // operand and the key errors e_p (public_key.rs:128-132) are drawn (or read) by the finish pass of the GEMM --
    // no transformed rows of either in memory.  l = 64: both through API-layout rows from one prologue launch.
    GemmSection ga{d_xm, d_erow, d_erow, d_tmp, cnt, 0, 0}, gb{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    ga.tiled_out = c->dB;
    ga.tiled_row0 = p0 - c->party_lo;
    ga.tiled_swap = 1;
    ga.row_stride = (size_t)k * P;
    if (direct) {
      draw.party0 = p0;
      PVW_HIP(launch_shat_mftile(ks.seeded() ? nullptr : d_small, ks.seeded() ? &draw : nullptr, d_xm, cnt, k, L, l, c->dt, s));
      GemmErrSource es{};
      if (ek) { es.explicit_coeffs = d_small + (size_t)chunk * k * l; es.coef_row = k; es.coef_v = 1; }
      else es.key[0] = make_key(seed);
      es.domain = DOM_EKEY; es.index0 = p0 * k; es.index_row = k; es.index_v = 1; es.bound = c->b1;
      ga.addend = nullptr;
      ga.out = nullptr;
      // all k columns in one launch (crs.rs:152-168)
      PVW_HIP(launch_gemm_digits(ga, gb, d_yd, d_sy, c->dt, k, L, l, k, P, 0, s, &es));
    } else {
      PrologueBatch pb{};
      if (seed) pb.key[0] = make_key(seed);
      PrologueJob& js = pb.job[0];
      PrologueJob& je = pb.job[1];
      PVW_TRY(ks.job(c, pb, js, d_small, p0));
      js.out = d_srow; js.stride_poly = P; js.stride_limb = l; js.rep_out = (size_t)k * P;
      je.sj.kind = SAMPLE_UNIFORM; je.sj.domain = DOM_EKEY; je.sj.index0 = p0 * k; je.sj.count = k; je.sj.bound = c->b1;
      je.rep_index0 = k;
      if (ek) { je.explicit_coeffs = d_small + (size_t)chunk * k * l; je.rep_coeffs = (size_t)k * l; }
      je.out = d_erow; je.stride_poly = P; je.stride_limb = l; je.rep_out = (size_t)k * P;
      pb.njobs = 2;
      pb.reps = cnt;
      PVW_HIP(launch_prologue(pb, c->dt, L, l, s));
      PVW_HIP(hipMemsetAsync(d_xm, 0, xm_words(cnt, k, L, l) * 8, s));
      PVW_HIP(launch_mftile(d_srow, false, d_xm, cnt, k, L, l, s));
      // out / addend element (v = col, row = p) at p * k * P + col * P
      PVW_HIP(launch_gemm_digits(ga, gb, d_yd, d_sy, c->dt, k, L, l, k, P, 0, s));
    }
    if (ks.seeded()) continue;
    PVW_HIP(hipEventRecord(w->events[2 * ci + 1], s));                         // this chunk's key buffer is free again
    if (ci + 1 < nchunks) {
      // issued after this chunk's launches so that the host-side staging of a pageable copy overlaps the GPU's work;
      // the buffer of chunk i+1 was last read by the prologue of chunk i-1
      if (ci >= 1) PVW_HIP(hipStreamWaitEvent(w->aux, w->events[2 * (ci - 1) + 1], 0));
      PVW_TRY(upload(ci + 1, w->aux));
      PVW_HIP(hipEventRecord(w->events[2 * ci + 2], w->aux));
    }
  }
  return PVW_OK;
}

// fewer than 64 parties, or PVW_KEYGEN_SWAP=0: the CRS transposed once per call and streamed, the parties' s-hat as the
// vectors -- 16 per pass on the matrix cores (everything around the GEMM batched over super-groups of up to 128 parties),
// 4 per pass on the VALU
static int32_t keygen_transposed(pvw_ctx* c, Workspace* w, u32 a, u32 b, u32 lo, const KeySource& ks, const int64_t* ek,
                                 const uint8_t* seed, bool use_gemm) {
  const u32 k = c->k, l = c->l, L = c->L;
  const size_t P = c->poly();
  hipStream_t s = w->stream;
  const u32 group = use_gemm ? 16 : 4;
  // super-group: parties whose sampling, NTTs, digit tiles and final tiling are single launches; bounded so
  // that the digit tiles stay below ~2 GiB
  u32 sg = group;
  if (use_gemm) {
    const size_t per16 = yd_bytes(16, k, L, l);
    size_t m = ((size_t)2 << 30) / (per16 ? per16 : 1);
    if (m < 1) m = 1;
    if (m > 8) m = 8;
    sg = 16 * (u32)m;
  }
  u32 chunk = (b - a) < 1024 ? (b - a) : 1024;         // parties whose sk / ek are uploaded together
  if (chunk > sg) chunk -= chunk % sg;                  // whole super-groups per chunk
  // scratch: A in API layout [k][k][P] | A^T in API layout | A^T tiled or MFMA-tiled | sk,ek of one chunk |
  //          rows of B for one super-group | gemm intermediate | (gemm) s-hat vectors, digit tiles, column sums
  Scratch sc;
  const size_t r_api = sc.add((size_t)k * k * P * 8), r_apiT = sc.add((size_t)k * k * P * 8);
  const size_t r_tt = sc.add((use_gemm ? xm_words(k, k, L, l) : c->tiled_words(k)) * 8);
  const size_t r_small = sc.add(ks.seeded() ? 0 : (size_t)2 * chunk * k * l * 8), r_row = sc.add((size_t)sg * k * P * 8);   // seeded: nothing is uploaded
  const size_t r_tmp = sc.add(use_gemm ? (size_t)(sg / 16) * gemm_tmp_words(k, L, l) * 8 : 0);
  const size_t r_vh = sc.add(use_gemm ? (size_t)sg * k * P * 8 : 0);
  const size_t r_yd = sc.add(use_gemm ? yd_bytes(sg, k, L, l) : 0), r_sy = sc.add(use_gemm ? sy_bytes(sg, L, l) : 0);
  PVW_TRY(sc.take(w));
  u64 *d_api = sc.at(r_api), *d_apiT = sc.at(r_apiT), *d_tt = sc.at(r_tt), *d_row = sc.at(r_row), *d_tmp = sc.at(r_tmp), *d_vh = sc.at(r_vh);
  i64* d_small = sc.at<i64>(r_small);
  signed char* d_yd = sc.at<signed char>(r_yd);
  int* d_sy = sc.at<int>(r_sy);
  // secret-bearing regions (cleared when the call ends): uploaded sk / ek coefficients; NTT(s) vectors, their digit
  // tiles and column sums (matrix-core form) or the s-hat vectors in w->rhat (VALU form).  d_row holds e only
  // until the product is added onto it, then rows of the public key.
  sc.secret(w, r_small, r_small);
  if (use_gemm) {
    sc.secret(w, r_tmp, r_tmp);                            // s A^T without the error
    sc.secret(w, r_vh, r_sy);
  }
  else ws_mark_secret(w, w->rhat, w->rhat_bytes);
  // A -> API layout -> transpose polynomials (A^T[c][j] = A[j][c]) -> tiled / MFMA-tiled
  PVW_HIP(launch_untile(c->dA, d_api, k, 0, k, L, l, false, c->dt, s));
  PVW_HIP(launch_transpose_polys(d_api, d_apiT, k, (u32)P, s));
  PVW_HIP(hipMemsetAsync(d_tt, 0, sc.bytes(r_tt), s));
  if (use_gemm) PVW_HIP(launch_mftile(d_apiT, false, d_tt, k, k, L, l, s));
  else PVW_HIP(launch_tile(d_apiT, d_tt, k, 0, k, L, l, false, c->dt, s));
  for (u32 p0 = a; p0 < b; p0 += sg) {
    const u32 nv = (b - p0) < sg ? (b - p0) : sg;
    const u32 in_chunk = (p0 - a) % chunk;                       // position inside the uploaded chunk
    if (in_chunk == 0 && !ks.seeded()) {
      const i64* sk = ks.sk;
      const u32 cn = (b - p0) < chunk ? (b - p0) : chunk;
      const size_t words = (size_t)cn * k * l;
      PVW_HIP(hipMemcpyAsync(d_small, sk + (size_t)(p0 - lo) * k * l, words * 8, hipMemcpyHostToDevice, s));
      if (ek) PVW_HIP(hipMemcpyAsync(d_small + (size_t)chunk * k * l, ek + (size_t)(p0 - lo) * k * l, words * 8, hipMemcpyHostToDevice, s));
    }
    ProfScope ps(c, "keygen", s);
    // ONE prologue launch for the super-group: the (s, e) families of party p0 replicated over its nv parties.  s-hat_p
    // (secret_key.rs:98-112) goes to the vector layout [party][limb][j][slot] (d_vh, or w->rhat on the VALU); e_p
    // (public_key.rs:128-132), sampled or explicit, to NTT form in the row buffer [nv][k][P]
    PrologueBatch pb{};
    if (seed) pb.key[0] = make_key(seed);
    PrologueJob& js = pb.job[0];
    PrologueJob& je = pb.job[1];
    u64* vh = use_gemm ? d_vh : w->rhat;
    PVW_TRY(ks.job(c, pb, js, d_small + (size_t)in_chunk * k * l, p0));
    js.out = vh; js.stride_poly = l; js.stride_limb = (size_t)k * l;
    js.rep_out = (size_t)k * P;
    je.sj.kind = SAMPLE_UNIFORM; je.sj.domain = DOM_EKEY; je.sj.index0 = p0 * k; je.sj.count = k; je.sj.bound = c->b1;
    je.rep_index0 = k;
    if (ek) { je.explicit_coeffs = d_small + (size_t)(chunk + in_chunk) * k * l; je.rep_coeffs = (size_t)k * l; }
    je.out = d_row; je.stride_poly = P; je.stride_limb = l; je.rep_out = (size_t)k * P;
    pb.njobs = 2;
    pb.reps = nv;
    PVW_HIP_AS(PVW_ERR_KEY_GENERATION, launch_prologue(pb, c->dt, L, l, s));
    if (use_gemm) {
      PVW_HIP_AS(PVW_ERR_KEY_GENERATION, launch_vec_digits(d_vh, (size_t)k * P, d_yd, d_sy, nv, k, L, l, c->dt, s));
      // all batches of 16 parties in one launch (crs.rs:152-168): they share A^T through L2
      // ... and the finish pass writes b_p = s_p*A + e_p straight into the tiled B-hat (no re-tiling launch)
      GemmSection ga{d_tt, d_row, d_row, d_tmp, k, 0, 0}, gb{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
      ga.tiled_out = c->dB;
      ga.tiled_row0 = p0 - c->party_lo;
      PVW_HIP_AS(PVW_ERR_KEY_GENERATION, launch_gemm_digits(ga, gb, d_yd, d_sy, c->dt, k, L, l, nv, (size_t)k * P, 0, s));
    } else {
      MacSection sa(d_tt, d_row, d_row, k), sb;
      MultiVec mv{vh, (size_t)k * P, (size_t)k * P, 0, nv};
      PVW_HIP_AS(PVW_ERR_KEY_GENERATION, launch_mac_rows_multi(sa, sb, mv, c->dt, k, L, l, s));
      // d_row is [nv][k polys][P] = nv rows of B in API layout -> tile into B
      PVW_HIP_AS(PVW_ERR_KEY_GENERATION, launch_tile(d_row, c->dB, nv, p0 - c->party_lo, k, L, l, false, c->dt, s));
    }
  }
  return PVW_OK;
}

// pvw_keygen and pvw_keygen_seeded behind their own NULL checks: one sequence of checks, one bookkeeping
static int32_t keygen_call(pvw_ctx* c, uint32_t lo, uint32_t hi, const KeySource& ks, const int64_t* ek, const uint8_t* seed) {
  PVW_TRY(check_party_range(c, lo, hi));
  if (ks.seeded()) PVW_TRY(check_sk_index(c, hi));
  PVW_TRY(ensure_device(c));
  matrix_changed(c, false);
  if (!c->crs_loaded) return fail(PVW_ERR_CRS, "CRS not loaded");
  if (c->rowsA() != c->k) return fail(PVW_ERR_KEY_GENERATION, "key generation needs the full CRS on this context");
  PVW_TRY(ensure_matrix(c, &c->dB, c->rowsB()));
  const u32 a = lo > c->party_lo ? lo : c->party_lo, b = hi < c->party_hi ? hi : c->party_hi;
  // >= 8 parties: the matrix cores (gemm_digits, 16 parties per pass); fewer: 4 per pass on the VALU
  const int gemm_min = (int)PVW_ENV_INT("PVW_GEMM_MIN_DEALERS", 8);   // tuning build only
  const bool use_gemm = gemm_min > 0 && (b - a) >= (u32)gemm_min;
  // default matrix-core form: parties as GEMM rows, the CRS columns digitised once (PVW_KEYGEN_SWAP=0: the earlier
  // form with the transposed CRS as the streamed operand and the secret keys digitised per super-group)
  const int swap_roles = (int)PVW_ENV_INT("PVW_KEYGEN_SWAP", 1);   // tuning build, per call: the tests walk both
  const int32_t rc = host_call(c, [&](Workspace* w) {
    return use_gemm && swap_roles && (b - a) >= 64 ? keygen_gemm_swapped(c, w, a, b, lo, ks, ek, seed)
                                                   : keygen_transposed(c, w, a, b, lo, ks, ek, seed, use_gemm);
  });
  if (rc == PVW_OK && hi > c->num_keys) c->num_keys = hi;
  return rc;
}
int32_t pvw_keygen(pvw_ctx* c, uint32_t lo, uint32_t hi, const int64_t* sk, const int64_t* ek, const uint8_t seed[32]) {
  if (!c || !sk) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!ek && !seed) return fail(PVW_ERR_INVALID_PARAMETERS, "either explicit key errors or a seed is required");
  KeySource ks;
  ks.sk = sk;
  return keygen_call(c, lo, hi, ks, ek, seed);
}
// GlobalPublicKey::generate_all_party_keys over Party::new / SecretKey::random (public_key.rs:376-401, :62-79,
// secret_key.rs:45-63): the keys are drawn where they are used and never exist on the host
int32_t pvw_keygen_seeded(pvw_ctx* c, uint32_t lo, uint32_t hi, const uint8_t sk_seed[32], const uint8_t seed[32]) {
  if (!c || !sk_seed || !seed) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  KeySource ks;
  ks.sk_seed = sk_seed;
  return keygen_call(c, lo, hi, ks, nullptr, seed);
}

// ------------------------------------------------------------------------ wire format, version 1
// Header: magic "PVWw", u16 version, u16 kind, u32 repr, u32 n k l L, f32 secret_variance, u64 error_bound_1 / _2, L x u64 moduli,
// [NTT bodies: L x u64 psi], row ranges as u32 pairs (CRS / public key: 1 pair, ciphertext: 2), u64 body_len, zero bytes up to a
// multiple of 16.  Body: packed polynomials (kinds 2-4), k*l i64 (kind 5), nothing (kind 1).
enum { WIRE_PARAMS = 1, WIRE_CRS = 2, WIRE_PK = 3, WIRE_CT = 4, WIRE_SK = 5 };
static const size_t WIRE_FIXED = 48;            // bytes before the moduli
static u32 wire_width(u64 q) {
  u32 b = 0;
  for (; q; q >>= 1) ++b;
  return b;
}
static size_t wire_poly_bytes(const pvw_ctx* c) {
  size_t s = 0;
  for (u64 q : c->moduli) s += wire_width(q);
  return s * c->l / 8;
}
static u32 wire_nranges(u32 kind) { return kind == WIRE_CT ? 2 : (kind == WIRE_CRS || kind == WIRE_PK ? 1 : 0); }
static size_t wire_header_len(const pvw_ctx* c, u32 kind, u32 repr) {
  size_t n = WIRE_FIXED + 8 * (size_t)c->L + (repr == PVW_REPR_NTT ? 8 * (size_t)c->L : 0) + 8 * wire_nranges(kind) + 8;
  return (n + 15) & ~(size_t)15;
}
// the body length of a (kind, repr, ranges) the context can hold, or an error
static int32_t wire_body_len(const pvw_ctx* c, u32 kind, u32 repr, const u32 r[4], size_t* out) {
  if (kind < WIRE_PARAMS || kind > WIRE_SK) return fail(PVW_ERR_INVALID_FORMAT, "wire: unknown kind " + std::to_string(kind));
  PVW_TRY(check_repr(repr));
  if ((kind == WIRE_PARAMS || kind == WIRE_SK) && repr != PVW_REPR_POWER)
    return fail(PVW_ERR_INVALID_FORMAT, "wire: parameters and secret keys carry repr POWER");
  const size_t pb = wire_poly_bytes(c);
  auto range = [&](u32 lo, u32 hi, u32 bound, const char* what) -> int32_t {
    if (lo > hi || hi > bound)
      return fail(PVW_ERR_INVALID_FORMAT, std::string("wire: ") + what + " range [" + std::to_string(lo) + ", " + std::to_string(hi) +
                                              ") outside [0, " + std::to_string(bound) + ")");
    return PVW_OK;
  };
  switch (kind) {
    case WIRE_PARAMS: *out = 0; break;
    case WIRE_SK: *out = (size_t)c->k * c->l * 8; break;
    case WIRE_CRS: PVW_TRY(range(r[0], r[1], c->k, "CRS row")); *out = (size_t)(r[1] - r[0]) * c->k * pb; break;
    case WIRE_PK: PVW_TRY(range(r[0], r[1], c->n, "public-key row")); *out = (size_t)(r[1] - r[0]) * c->k * pb; break;
    default:
      PVW_TRY(range(r[0], r[1], c->k, "c1 row"));
      PVW_TRY(range(r[2], r[3], c->n, "c2 row"));
      *out = ((size_t)(r[1] - r[0]) + (r[3] - r[2])) * pb;
  }
  return PVW_OK;
}
static void le_put(uint8_t* p, u64 v, int bytes) {
  for (int i = 0; i < bytes; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
static u64 le_get(const uint8_t* p, int bytes) {
  u64 v = 0;
  for (int i = 0; i < bytes; ++i) v |= (u64)p[i] << (8 * i);
  return v;
}
static u32 f32_bits(float f) {
  u32 b;
  memcpy(&b, &f, 4);
  return b;
}

// host codec (plain C++, the reference implementation of the format)
static void wire_pack_one(const pvw_ctx* c, const u64* poly, uint8_t* out) {
  u128 acc = 0;
  u32 nb = 0;
  size_t o = 0;
  for (u32 i = 0; i < c->L; ++i) {
    const u64 q = c->moduli[i];
    const u32 w = wire_width(q);
    for (u32 j = 0; j < c->l; ++j) {
      acc |= (u128)(poly[(size_t)i * c->l + j] % q) << nb;
      nb += w;
      while (nb >= 8) {
        out[o++] = (uint8_t)acc;
        acc >>= 8;
        nb -= 8;
      }
    }
  }
}
// returns the number of fields >= q_i; *first = limb * l + slot of the first one
static size_t wire_unpack_one(const pvw_ctx* c, const uint8_t* in, u64* poly, size_t* first) {
  u128 acc = 0;
  u32 nb = 0;
  size_t o = 0, bad = 0;
  for (u32 i = 0; i < c->L; ++i) {
    const u64 q = c->moduli[i];
    const u32 w = wire_width(q);
    for (u32 j = 0; j < c->l; ++j) {
      while (nb < w) {
        acc |= (u128)in[o++] << nb;
        nb += 8;
      }
      const u64 v = (u64)acc & ((1ull << w) - 1);
      acc >>= w;
      nb -= w;
      if (poly) poly[(size_t)i * c->l + j] = v;
      if (v >= q && bad++ == 0 && first) *first = (size_t)i * c->l + j;
    }
  }
  return bad;
}
static int32_t wire_reject(const pvw_ctx* c, size_t poly, size_t at, const uint8_t* in) {
  std::vector<u64> words(c->poly());
  wire_unpack_one(c, in, words.data(), nullptr);
  const u32 limb = (u32)(at / c->l), slot = (u32)(at % c->l);
  char buf[200];
  snprintf(buf, sizeof buf, "wire: residue out of range at polynomial %zu, limb %u, slot %u (field %llu >= q_%u = %llu)", poly, limb,
           slot, (unsigned long long)words[at], limb, (unsigned long long)c->moduli[limb]);
  return fail(PVW_ERR_DESERIALIZATION, buf);
}
// first rejected residue among `count` packed polynomials on the host (the error path of the device readers)
static int32_t wire_find_reject(const pvw_ctx* c, const uint8_t* in, size_t count, size_t poly0) {
  const size_t pb = wire_poly_bytes(c);
  for (size_t p = 0; p < count; ++p) {
    size_t at = 0;
    if (wire_unpack_one(c, in + p * pb, nullptr, &at)) return wire_reject(c, poly0 + p, at, in + p * pb);
  }
  return fail(PVW_ERR_DESERIALIZATION, "wire: residues out of range (the host rescan found none: was the input changed meanwhile?)");
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int32_t wire_device_checks(const pvw_ctx* c) {
  if (c->L > 64) return fail(PVW_ERR_INVALID_PARAMETERS, "the device wire codec takes at most 64 moduli");
  return PVW_OK;
}
// polynomials per staging chunk: a multiple of 16 (every chunk starts 16-byte aligned in both forms), about `bytes` of words
static size_t wire_chunk_polys(const pvw_ctx* c, size_t bytes) {
  size_t n = bytes / (c->poly() * 8) / 16 * 16;
  return n ? n : 16;
}
static int32_t wire_pack_enqueue(pvw_ctx* c, const u64* d_polys, size_t count, uint8_t* d_out, hipStream_t s) {
  ProfScope ps(c, "wire_pack", s);
  PVW_HIP(launch_wire_pack(d_polys, count, d_out, c->dt.mods, c->L, c->l, s));
  return PVW_OK;
}
static int32_t wire_unpack_enqueue(pvw_ctx* c, const uint8_t* d_in, size_t count, u64* d_polys, u64* d_bad, hipStream_t s) {
  ProfScope ps(c, "wire_unpack", s);
  PVW_HIP(launch_wire_unpack(d_in, count, d_polys, (unsigned long long*)d_bad, c->dt.mods, c->L, c->l, s));
  return PVW_OK;
}

// rows [lo, hi) of a matrix (k polynomials a row) from a packed host body: every row the shard holds is staged and checked
// before any of them is unpacked, so a rejected body leaves the resident matrix as it was.  `commit` runs between the two
// (invalidates the derived copies, allocates the matrix).  Bodies up to 1 GiB are staged whole; larger ones are read twice.
static int32_t wire_load_rows(pvw_ctx* c, u64** Mp, u32 shard_lo, u32 shard_hi, u32 lo, u32 hi, const uint8_t* body, uint32_t repr,
                              const std::function<int32_t()>& commit) {
  const u32 a = lo > shard_lo ? lo : shard_lo, b = hi < shard_hi ? hi : shard_hi;
  if (a >= b) return commit();
  const size_t k = c->k, pb = wire_poly_bytes(c), rowbytes = k * pb, rowwords = k * c->poly();
  const u32 m = 16 / (u32)(k & 15 ? (k & 1 ? 1 : (k & 3 ? 2 : (k & 7 ? 4 : 8))) : 16);   // rows of a 16-polynomial multiple
  const uint8_t* src = body + (size_t)(a - lo) * rowbytes;
  const size_t total = (size_t)(b - a) * rowbytes;
  const bool whole = total <= ((size_t)1 << 30);
  size_t stage_rows = whole ? (size_t)(b - a) : ((size_t)256 << 20) / rowbytes / m * m;
  if (stage_rows == 0) stage_rows = m;
  size_t word_rows = ((size_t)256 << 20) / (rowwords * 8) / m * m;
  if (word_rows == 0) word_rows = m;
  // the staged body and the check count behind it, outside the pooled scratch (which takes the unpacked words)
  Scratch st(16);
  const size_t r_pk = st.add(stage_rows * rowbytes), r_bad = st.add(8);
  if (hipMalloc((void**)&st.base, st.total) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PVW_ERR_INTERNAL, "wire: no device memory for the staged body");
  }
  uint8_t* d_pk = st.at<uint8_t>(r_pk);
  u64* d_bad = st.at(r_bad);
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    auto stage = [&](u32 r0, u32 cnt) {
      return hipMemcpyAsync(d_pk, src + (size_t)(r0 - a) * rowbytes, (size_t)cnt * rowbytes, hipMemcpyHostToDevice, w->stream);
    };
    // pass 1: check
    PVW_HIP(hipMemsetAsync(d_bad, 0, 8, w->stream));
    for (u32 r0 = a; r0 < b; r0 += (u32)stage_rows) {
      const u32 cnt = (size_t)(b - r0) < stage_rows ? (b - r0) : (u32)stage_rows;
      PVW_HIP(stage(r0, cnt));
      PVW_TRY(wire_unpack_enqueue(c, d_pk, (size_t)cnt * k, nullptr, d_bad, w->stream));
    }
    u64 bad = 0;
    PVW_HIP(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, w->stream));
    PVW_HIP(hipStreamSynchronize(w->stream));
    if (bad) return wire_find_reject(c, src, (size_t)(b - a) * k, (size_t)(a - lo) * k);
    // pass 2: unpack and tile
    PVW_TRY(commit());
    PVW_TRY(ws_scratch(w, word_rows * rowwords * 8));
    for (u32 r0 = a; r0 < b; r0 += (u32)stage_rows) {
      const u32 cnt = (size_t)(b - r0) < stage_rows ? (b - r0) : (u32)stage_rows;
      if (!whole) PVW_HIP(stage(r0, cnt));
      for (u32 s0 = 0; s0 < cnt; s0 += (u32)word_rows) {
        const u32 sc = (size_t)(cnt - s0) < word_rows ? (cnt - s0) : (u32)word_rows;
        PVW_TRY(wire_unpack_enqueue(c, d_pk + (size_t)s0 * rowbytes, (size_t)sc * k, (u64*)w->scratch, d_bad, w->stream));
        PVW_TRY(load_rows_device(c, *Mp, shard_lo, shard_hi, r0 + s0, r0 + s0 + sc, (const u64*)w->scratch, repr, w->stream));
      }
    }
    return PVW_OK;
  });
  hipFree(st.base);
  return rc;
}
// rows [lo, hi) of a resident matrix, packed, to a host body (rows the shard does not hold are not written)
static int32_t wire_get_rows(pvw_ctx* c, const u64* M, u32 shard_lo, u32 shard_hi, u32 lo, u32 hi, uint8_t* body, uint32_t repr) {
  const u32 a = lo > shard_lo ? lo : shard_lo, b = hi < shard_hi ? hi : shard_hi;
  if (a >= b) return PVW_OK;
  if (!M) return fail(PVW_ERR_INVALID_PARAMETERS, "matrix not loaded");
  const size_t k = c->k, pb = wire_poly_bytes(c), rowbytes = k * pb, rowwords = k * c->poly();
  const u32 m = 16 / (u32)(k & 15 ? (k & 1 ? 1 : (k & 3 ? 2 : (k & 7 ? 4 : 8))) : 16);
  size_t chunk = ((size_t)256 << 20) / (rowwords * 8) / m * m;
  if (chunk == 0) chunk = m;
  Scratch sc(16);
  const size_t r_w = sc.add(chunk * rowwords * 8), r_pk = sc.add(chunk * rowbytes);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    for (u32 r0 = a; r0 < b; r0 += (u32)chunk) {
      const u32 cnt = (size_t)(b - r0) < chunk ? (b - r0) : (u32)chunk;
      PVW_HIP(launch_untile(M, sc.at(r_w), cnt, r0 - shard_lo, c->k, c->L, c->l, repr == PVW_REPR_POWER, c->dt, w->stream));
      PVW_TRY(wire_pack_enqueue(c, sc.at(r_w), (size_t)cnt * k, sc.at<uint8_t>(r_pk), w->stream));
      PVW_HIP(hipMemcpyAsync(body + (size_t)(r0 - lo) * rowbytes, sc.at<uint8_t>(r_pk), (size_t)cnt * rowbytes, hipMemcpyDeviceToHost, w->stream));
    }
    return PVW_OK;
  });
}

int32_t pvw_wire_poly_bytes(const pvw_ctx* c, size_t* out) {
  if (!c || !out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  *out = wire_poly_bytes(c);
  return PVW_OK;
}

int32_t pvw_wire_header(const pvw_ctx* c, uint32_t kind, uint32_t repr, uint32_t lo, uint32_t hi, uint32_t lo2, uint32_t hi2,
                        uint8_t* out, size_t cap, size_t* len) {
  if (!c || !len) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const u32 r[4] = {lo, hi, lo2, hi2};
  size_t body = 0;
  PVW_TRY(wire_body_len(c, kind, repr, r, &body));
  const size_t hl = wire_header_len(c, kind, repr);
  *len = hl;
  if (!out) return PVW_OK;
  if (cap < hl) return fail(PVW_ERR_SERIALIZATION, "wire: header buffer holds " + std::to_string(cap) + " bytes, needs " + std::to_string(hl));
  memset(out, 0, hl);
  memcpy(out, "PVWw", 4);
  le_put(out + 4, 1, 2);
  le_put(out + 6, kind, 2);
  le_put(out + 8, repr, 4);
  le_put(out + 12, c->n, 4);
  le_put(out + 16, c->k, 4);
  le_put(out + 20, c->l, 4);
  le_put(out + 24, c->L, 4);
  le_put(out + 28, f32_bits(c->variance), 4);
  le_put(out + 32, c->b1, 8);
  le_put(out + 40, c->b2, 8);
  uint8_t* p = out + WIRE_FIXED;
  for (u64 q : c->moduli) { le_put(p, q, 8); p += 8; }
  if (repr == PVW_REPR_NTT)
    for (u64 psi : c->psi) { le_put(p, psi, 8); p += 8; }
  for (u32 i = 0; i < 2 * wire_nranges(kind); ++i) { le_put(p, r[i], 4); p += 4; }
  le_put(p, body, 8);
  return PVW_OK;
}

int32_t pvw_wire_header_check(const pvw_ctx* c, const uint8_t* in, size_t len, uint32_t* kind_out, uint32_t* repr_out,
                              uint32_t* ranges, size_t* header_len) {
  if (!c || !in) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (len < WIRE_FIXED) return fail(PVW_ERR_INVALID_FORMAT, "wire: truncated header (" + std::to_string(len) + " bytes)");
  if (memcmp(in, "PVWw", 4) != 0) return fail(PVW_ERR_INVALID_FORMAT, "wire: bad magic");
  const u32 version = (u32)le_get(in + 4, 2), kind = (u32)le_get(in + 6, 2), repr = (u32)le_get(in + 8, 4);
  if (version != 1) return fail(PVW_ERR_INVALID_FORMAT, "wire: unsupported version " + std::to_string(version));
  if (kind < WIRE_PARAMS || kind > WIRE_SK) return fail(PVW_ERR_INVALID_FORMAT, "wire: unknown kind " + std::to_string(kind));
  const char* names[4] = {"n", "k", "l", "L"};
  const u32 mine[4] = {c->n, c->k, c->l, c->L};
  for (int f = 0; f < 4; ++f) {
    const u32 v = (u32)le_get(in + 12 + 4 * f, 4);
    if (v != mine[f]) {
      char buf[120];
      snprintf(buf, sizeof buf, "wire: parameter %s differs: expected %u, actual %u", names[f], mine[f], v);
      return fail(PVW_ERR_DIMENSION_MISMATCH, buf);
    }
  }
  if ((u32)le_get(in + 28, 4) != f32_bits(c->variance) || le_get(in + 32, 8) != c->b1 || le_get(in + 40, 8) != c->b2)
    return fail(PVW_ERR_INVALID_FORMAT, "wire: the blob was written for other parameters (variance or error bounds differ)");
  if (repr != PVW_REPR_POWER && repr != PVW_REPR_NTT) return fail(PVW_ERR_INVALID_FORMAT, "wire: unknown representation");
  const size_t hl = wire_header_len(c, kind, repr);
  if (len < hl) return fail(PVW_ERR_INVALID_FORMAT, "wire: truncated header (" + std::to_string(len) + " of " + std::to_string(hl) + " bytes)");
  const uint8_t* p = in + WIRE_FIXED;
  for (u32 i = 0; i < c->L; ++i, p += 8)
    if (le_get(p, 8) != c->moduli[i]) return fail(PVW_ERR_INVALID_FORMAT, "wire: the blob was written for other moduli (q_" + std::to_string(i) + ")");
  if (repr == PVW_REPR_NTT)
    for (u32 i = 0; i < c->L; ++i, p += 8)
      if (le_get(p, 8) != c->psi[i])
        return fail(PVW_ERR_INVALID_FORMAT, "wire: NTT-domain body under other roots (psi_" + std::to_string(i) + " differs from this context's)");
  u32 r[4] = {0, 0, 0, 0};
  for (u32 i = 0; i < 2 * wire_nranges(kind); ++i, p += 4) r[i] = (u32)le_get(p, 4);
  size_t body = 0;
  PVW_TRY(wire_body_len(c, kind, repr, r, &body));
  if (le_get(p, 8) != body) return fail(PVW_ERR_INVALID_FORMAT, "wire: body_len does not match the kind and row ranges");
  for (const uint8_t* z = p + 8; z < in + hl; ++z)
    if (*z) return fail(PVW_ERR_INVALID_FORMAT, "wire: header padding is not zero");
  if (len < hl + body) return fail(PVW_ERR_INVALID_FORMAT, "wire: truncated body (" + std::to_string(len - hl) + " of " + std::to_string(body) + " bytes)");
  if (len > hl + body) return fail(PVW_ERR_INVALID_FORMAT, "wire: " + std::to_string(len - hl - body) + " trailing bytes");
  if (kind_out) *kind_out = kind;
  if (repr_out) *repr_out = repr;
  if (ranges) memcpy(ranges, r, sizeof r);
  if (header_len) *header_len = hl;
  return PVW_OK;
}

int32_t pvw_wire_pack_host(const pvw_ctx* c, const uint64_t* polys, size_t count, uint8_t* out) {
  if (!c || ((!polys || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const size_t pb = wire_poly_bytes(c), P = c->poly();
  if (count) memset(out, 0, count * pb);
  for (size_t p = 0; p < count; ++p) wire_pack_one(c, polys + p * P, out + p * pb);
  return PVW_OK;
}

int32_t pvw_wire_unpack_host(const pvw_ctx* c, const uint8_t* in, size_t count, uint64_t* polys, uint64_t* bad_out) {
  if (!c || ((!polys || !in) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  const size_t pb = wire_poly_bytes(c), P = c->poly();
  size_t bad = 0, first_poly = 0, first_at = 0;
  for (size_t p = 0; p < count; ++p) {
    size_t at = 0;
    const size_t nb = wire_unpack_one(c, in + p * pb, polys + p * P, &at);
    if (nb && !bad) { first_poly = p; first_at = at; }
    bad += nb;
  }
  if (bad_out) *bad_out = bad;
  return bad ? wire_reject(c, first_poly, first_at, in + first_poly * pb) : PVW_OK;
}

int32_t pvw_wire_pack_device(pvw_ctx* c, const uint64_t* d_polys, size_t count, uint8_t* d_out, void* stream) {
  if (!c || ((!d_polys || !d_out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!aligned16(d_polys) || !aligned16(d_out)) return fail(PVW_ERR_INVALID_PARAMETERS, "wire: device buffers must be 16-byte aligned");
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  return wire_pack_enqueue(c, d_polys, count, d_out, call_stream(c, stream));
}

int32_t pvw_wire_unpack_device(pvw_ctx* c, const uint8_t* d_in, size_t count, uint64_t* d_polys, uint64_t* d_bad, void* stream) {
  if (!c || !d_bad || ((!d_in || !d_polys) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  if (!aligned16(d_in) || !aligned16(d_polys)) return fail(PVW_ERR_INVALID_PARAMETERS, "wire: device buffers must be 16-byte aligned");
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  hipStream_t s = call_stream(c, stream);
  PVW_HIP(hipMemsetAsync(d_bad, 0, 8, s));
  return wire_unpack_enqueue(c, d_in, count, d_polys, d_bad, s);
}

int32_t pvw_wire_pack(pvw_ctx* c, const uint64_t* polys, size_t count, uint8_t* out) {
  if (!c || ((!polys || !out) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(wire_device_checks(c));
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const size_t pb = wire_poly_bytes(c), P = c->poly(), chunk = wire_chunk_polys(c, (size_t)256 << 20);
  // output the device can write (pvw_host_alloc, or pinned / registered by the caller): the kernel stores into it directly
  uint8_t* direct = (uint8_t*)device_alias(out, count * pb);
  if (direct && !aligned16(direct)) direct = nullptr;
  const size_t n0 = count < chunk ? count : chunk;
  Scratch sc(16);
  const size_t r_w = sc.add(n0 * P * 8), r_pk = sc.add(n0 * pb);
  return host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    for (size_t p0 = 0; p0 < count; p0 += chunk) {
      const size_t cnt = count - p0 < chunk ? count - p0 : chunk;
      uint8_t* d_pk = direct ? direct + p0 * pb : sc.at<uint8_t>(r_pk);
      PVW_HIP(hipMemcpyAsync(sc.at(r_w), polys + p0 * P, cnt * P * 8, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(wire_pack_enqueue(c, sc.at(r_w), cnt, d_pk, w->stream));
      if (!direct) PVW_HIP(hipMemcpyAsync(out + p0 * pb, d_pk, cnt * pb, hipMemcpyDeviceToHost, w->stream));
    }
    return PVW_OK;
  });
}

int32_t pvw_wire_unpack(pvw_ctx* c, const uint8_t* in, size_t count, uint64_t* polys) {
  if (!c || ((!polys || !in) && count)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(wire_device_checks(c));
  if (!count) return PVW_OK;
  PVW_TRY(ensure_device(c));
  const size_t pb = wire_poly_bytes(c), P = c->poly(), chunk = wire_chunk_polys(c, (size_t)256 << 20);
  const size_t n0 = count < chunk ? count : chunk;
  Scratch sc(16);
  const size_t r_w = sc.add(n0 * P * 8), r_pk = sc.add(n0 * pb), r_bad = sc.add(8);
  u64 bad = 0;                                    // residues >= q_i over all chunks
  const int32_t rc = host_call(c, [&](Workspace* w) -> int32_t {
    PVW_TRY(sc.take(w));
    PVW_HIP(hipMemsetAsync(sc.at(r_bad), 0, 8, w->stream));
    for (size_t p0 = 0; p0 < count; p0 += chunk) {
      const size_t cnt = count - p0 < chunk ? count - p0 : chunk;
      PVW_HIP(hipMemcpyAsync(sc.at<uint8_t>(r_pk), in + p0 * pb, cnt * pb, hipMemcpyHostToDevice, w->stream));
      PVW_TRY(wire_unpack_enqueue(c, sc.at<uint8_t>(r_pk), cnt, sc.at(r_w), sc.at(r_bad), w->stream));
      PVW_HIP(hipMemcpyAsync(polys + p0 * P, sc.at(r_w), cnt * P * 8, hipMemcpyDeviceToHost, w->stream));
    }
    PVW_HIP(hipMemcpyAsync(&bad, sc.at(r_bad), 8, hipMemcpyDeviceToHost, w->stream));
    return PVW_OK;
  });
  if (rc == PVW_OK && bad) return wire_find_reject(c, in, count, 0);
  return rc;
}

int32_t pvw_load_pk_wire(pvw_ctx* c, uint32_t lo, uint32_t hi, const uint8_t* body, uint32_t repr) {
  if (!c || (!body && lo != hi)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(check_party_range(c, lo, hi));
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  PVW_TRY(wire_load_rows(c, &c->dB, c->party_lo, c->party_hi, lo, hi, body, repr, [&]() -> int32_t {
    matrix_changed(c, false);
    return ensure_matrix(c, &c->dB, c->rowsB());
  }));
  if (hi > c->num_keys) c->num_keys = hi;                                          // public_key.rs:245-247
  return PVW_OK;
}

int32_t pvw_get_pk_wire(pvw_ctx* c, uint32_t lo, uint32_t hi, uint8_t* body_out, uint32_t repr) {
  if (!c || (!body_out && lo != hi)) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(check_party_range(c, lo, hi));
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  return wire_get_rows(c, c->dB, c->party_lo, c->party_hi, lo, hi, body_out, repr);
}

int32_t pvw_load_crs_wire(pvw_ctx* c, const uint8_t* body, uint32_t repr) {
  if (!c || !body) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  PVW_TRY(wire_load_rows(c, &c->dA, c->c1_lo, c->c1_hi, 0, c->k, body, repr, [&]() -> int32_t {
    matrix_changed(c, true);
    return ensure_matrix(c, &c->dA, c->rowsA());
  }));
  c->crs_loaded = true;
  return PVW_OK;
}

int32_t pvw_get_crs_wire(pvw_ctx* c, uint8_t* body_out, uint32_t repr) {
  if (!c || !body_out) return fail(PVW_ERR_INVALID_PARAMETERS, "NULL argument");
  PVW_TRY(check_repr(repr));
  PVW_TRY(wire_device_checks(c));
  PVW_TRY(ensure_device(c));
  return wire_get_rows(c, c->dA, c->c1_lo, c->c1_hi, 0, c->k, body_out, repr);
}

}  // extern "C"
