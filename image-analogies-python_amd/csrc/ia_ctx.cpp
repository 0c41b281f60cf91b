// ia_ctx.cpp — the context of libia.so: the thread's last error, ia_init / ia_destroy, the
// options (one table), the level-pipelining links between contexts, and the process-wide budget
// of handoff-chained waves with the pure helpers that size it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ia_host.h"

namespace ia_host {

static thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

// Waves of the handoff-chained launches (k_merge_gather: a gather waits for the merge of the row
// above) of every level in flight in this process.  A wave waits only for its row predecessor
// and no two waves share one, so a stall needs every resident slot held by a waiter whose
// predecessor is not yet dispatched: >= 2 x the resident slots chained waves in flight at once.
// The resident slots come from the compiled k_merge_gather instances (ia_chain_budget, at
// ia_init: VGPRs and the occupancy API; 4 waves per CU at round 4's 264 VGPRs).  A level
// chains only if its widest launch fits in the budget left (ia_synthesize_levels is
// synchronous: its launches are done when it returns); otherwise it runs the separate gather /
// merge launches.  (cfg5's 16-job batches of 512^2 steps, 2,736 waves per launch on three
// streams, hit the 20 s handoff timeout without this.)
// Two-wave workgroups (option "gather_wave"): a workgroup is dispatched whole, so a gather wave's
// own merge wave is always resident beside it; a gather wave waits only for that merge wave (one
// workgroup barrier) and for the slot of the row above, published by the MERGE wave of a
// workgroup with a lower index, dispatched before it; merge waves wait for nothing, so they
// always finish, release their gather waves, and the waits drain in index order as before.  Such
// a level holds two resident slots per query and reserves twice its waves (ia_chain_choice).
static std::atomic<int> g_chain_waves{0};
ChainReservation::~ChainReservation() {
  if (n) g_chain_waves.fetch_sub(n);
}
bool ChainReservation::take(int w, int budget) {
  int cur = g_chain_waves.load();
  while (cur + w <= budget)
    if (g_chain_waves.compare_exchange_weak(cur, cur + w)) {
      n = w;
      return true;
    }
  return false;
}
int chain_waves_in_flight() { return g_chain_waves.load(); }

}  // namespace ia_host

using namespace ia_host;

extern "C" {

const char *ia_last_error(void) { return g_last_error.c_str(); }
int ia_version(void) { return 4; }

int ia_init(int device, ia_ctx **out) {
  if (!out) return fail(IA_EINVAL, "ia_init: out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(IA_ENODEV, "ia_init: no HIP device visible");
  if (device < 0 || device >= n) return fail(IA_EINVAL, "ia_init: device index out of range");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(IA_ENODEV, std::string("ia_init: libia is built for gfx950 only, device is ") + prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  ia_ctx *c = new ia_ctx();
  c->dev = device;
  // IA_CU_SPLIT=k/n (rehearsals of the multi-rank exchanges with n ranks sharing ONE GPU only):
  // this context's stream runs on CU slice k of n, so a rank's kernel that waits for a peer's
  // progress never holds the CUs the peer's kernels need (on separate GPUs nothing is shared)
  int split_k = 0, split_n = 0;
  if (const char *e = std::getenv("IA_CU_SPLIT")) {
    if (std::sscanf(e, "%d/%d", &split_k, &split_n) != 2 || split_n < 1 || split_k < 0 || split_k >= split_n) split_n = 0;
  }
  hipError_t se;
  if (split_n > 1) {
    const int ncu = prop.multiProcessorCount;
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int cu = ncu * split_k / split_n; cu < ncu * (split_k + 1) / split_n; cu++) mask[cu / 32] |= 1u << (cu % 32);
    se = hipExtStreamCreateWithCUMask(&c->st, (uint32_t)mask.size(), mask.data());
  } else {
    se = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking);
  }
  if (se != hipSuccess) {
    delete c;
    return fail(IA_EHIP, "ia_init: hipStreamCreate failed");
  }
  {  // g_chain_waves: the resident k_merge_gather waves of this context's CU slice, twice, less 1/16
    const int ncu = split_n > 1 ? prop.multiProcessorCount / split_n : prop.multiProcessorCount;
    int vg = 0, nb = 0, wt = 0;
    ia_merge_gather_occupancy(&vg, &nb, &wt);
    c->chain_budget = ia_chain_budget(ncu, vg, nb, wt);  // 0: never chain (separate launches)
  }
  hipEventCreate(&c->lv0);
  hipEventCreate(&c->lv1);
  hipEventCreate(&c->lv2);
  for (hipEvent_t &e : c->kb) hipEventCreate(&e);
  *out = c;
  return IA_OK;
}

void ia_destroy(ia_ctx *c) {
  if (!c) return;
  hipSetDevice(c->dev);
  hipStreamSynchronize(c->st);
  for (auto *v : {&c->evs, &c->evg, &c->evm, &c->p_ev[0], &c->p_ev[1], &c->p_ev[2]})
    for (hipEvent_t e : *v) hipEventDestroy(e);
  for (hipEvent_t e : c->kb) hipEventDestroy(e);
  hipEventDestroy(c->lv0);
  hipEventDestroy(c->lv1);
  hipEventDestroy(c->lv2);
  comm_close(c);
  if (c->xbuf) hipFree(c->xbuf);
  if (c->hand) hipFree(c->hand);
  if (c->kslot) hipFree(c->kslot);
  const hipStream_t st = c->st;
  delete c;  // frees every DevBuf of the context: before the stream goes, as ever
  hipStreamDestroy(st);
}

// The options of ia_set_option, one row each: where the value is stored and what is accepted.
struct Option {
  const char *name;
  int ia_ctx::*at;  // nullptr: ia_set_option acts on it itself
  enum { FLAG, RANGE, LIST, WGS, MIN1, ANY } kind;  // 0 / 1; v[0]..v[1]; one of v[0..n); a multiple of 8 in
  int n, v[5];                                      // [8, IA_NWG_H]; >= 1; unchecked
};
static const Option OPTIONS[] = {
    {"time_dist", &ia_ctx::time_dist, Option::ANY},
    {"rec_wt", &ia_ctx::rec_wt, Option::FLAG},
    {"stamps", &ia_ctx::stamps, Option::FLAG},
    {"k3p_variant", &ia_ctx::k3p_variant, Option::LIST, 5, {20, 21, 22, 24, 25}},
    {"k3_variant", nullptr, Option::LIST, 1, {1}},  // stores nothing (the other epilogues are in git history)
    {"prune_group", &ia_ctx::prune_group, Option::LIST, 4, {1, 2, 4, 8}},
    {"prune_min_rows", nullptr, Option::MIN1},  // an int64_t member
    {"row_source", &ia_ctx::row_source, Option::LIST, 1, {0}},
    {"shard_emulate", &ia_ctx::shard_emulate, Option::RANGE, 2, {1, 64}},
    {"prune", &ia_ctx::prune, Option::FLAG},
    {"shard_unpruned", &ia_ctx::shard_unpruned, Option::FLAG},
    {"k3p_blocks", &ia_ctx::k3p_blocks, Option::FLAG},
    {"fuse_gather", &ia_ctx::fuse_gather, Option::FLAG},
    {"nn_bound", &ia_ctx::nn_bound, Option::FLAG},
    {"early_gather", &ia_ctx::early_gather, Option::FLAG},
    {"gather_wave", &ia_ctx::gather_wave, Option::FLAG},
    {"prefetch_next", &ia_ctx::prefetch_next, Option::FLAG},
    {"fuse_sort", &ia_ctx::fuse_sort, Option::RANGE, 2, {0, 2}},
    {"fuse_unpruned", &ia_ctx::fuse_unpruned, Option::FLAG},
    {"pipeline_last", &ia_ctx::p_last, Option::FLAG},
    {"pipeline_record", &ia_ctx::p_record, Option::FLAG},
    {"stream_priority", nullptr, Option::RANGE, 2, {0, 2}},  // recreates the stream
    {"scan_wgs", &ia_ctx::scan_wgs, Option::WGS},
    {"xo_wait", &ia_ctx::xo_wait, Option::FLAG},
    {"xo_presort", &ia_ctx::xo_presort, Option::FLAG},
    {"exchange", &ia_ctx::exchange, Option::RANGE, 2, {0, 2}},
    {"matcher", &ia_ctx::matcher, Option::FLAG},  // IA_MATCH_F32 / IA_MATCH_F16X3
};
// what o accepts, for the refusal of v; "" when it accepts v
static std::string refusal(const Option &o, int v) {
  std::string s;
  switch (o.kind) {
    case Option::FLAG: return v == 0 || v == 1 ? "" : "0 or 1";
    case Option::RANGE: return v >= o.v[0] && v <= o.v[1] ? "" : std::to_string(o.v[0]) + ".." + std::to_string(o.v[1]);
    case Option::LIST:
      for (int i = 0; i < o.n; i++) s += (i ? ", " : "one of ") + std::to_string(o.v[i]);
      return std::find(o.v, o.v + o.n, v) != o.v + o.n ? "" : s;
    case Option::WGS: return v >= 8 && v <= IA_NWG_H && v % 8 == 0 ? "" : "a multiple of 8 in [8, " + std::to_string(IA_NWG_H) + "]";
    case Option::MIN1: return v >= 1 ? "" : ">= 1";
    default: return "";  // ANY
  }
}

int ia_set_option(ia_ctx *c, const char *name, int value) {
  if (!c || !name) return fail(IA_EINVAL, "ia_set_option: NULL argument");
  const Option *o = std::find_if(std::begin(OPTIONS), std::end(OPTIONS), [&](const Option &x) { return !std::strcmp(name, x.name); });
  if (o == std::end(OPTIONS)) return fail(IA_EINVAL, std::string("ia_set_option: unknown option ") + name);
  const std::string want = refusal(*o, value);
  if (!want.empty()) return fail(IA_EINVAL, std::string("ia_set_option: ") + name + " must be " + want);
  if (o->at) c->*o->at = value;
  if (!std::strcmp(name, "prune_min_rows")) c->prune_min_rows = value;
  if (!std::strcmp(name, "stream_priority")) {
    // 0 = default, 1 = high, 2 = low: the stream is recreated (idle contexts only); level pipelining (DESIGN.md
    // §6b) runs the finest level's context high, so the coarser levels' kernels fill its gaps, not delay its steps
    if (std::getenv("IA_CU_SPLIT")) return fail(IA_EINVAL, "ia_set_option: stream_priority with IA_CU_SPLIT");
    HIP_TRY(hipSetDevice(c->dev));
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamSynchronize(c->st));
    hipStream_t ns = nullptr;
    HIP_TRY(hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, value == 0 ? 0 : value == 1 ? greatest : least));
    hipStreamDestroy(c->st);
    c->st = ns;
  }
  return IA_OK;
}

int ia_pipeline_depend(ia_ctx *c, ia_ctx *prev, int prev_gen) {
  if (!c || (prev && (prev == c || !prev->p_record || prev_gen < 1)))
    return fail(IA_EINVAL, "ia_pipeline_depend: prev must be another context with pipeline_record = 1 and prev_gen >= 1");
  c->dep = prev;
  c->dep_gen = prev ? prev_gen : 0;
  return IA_OK;
}

int ia_pipeline_generation(ia_ctx *c) { return c ? c->p_gen.load() : -1; }

int ia_chain_budget(int n_cu, int vgprs, int api_blocks_per_cu, int wg_threads) {
  // resident waves per CU: the VGPR bound (512 registers per lane and SIMD, allocated in
  // granules of 8, at most 8 waves per SIMD, 4 SIMDs) and the occupancy API's workgroups; above
  // 3 waves per SIMD the SGPR file can bind too, where the API is known to answer one workgroup
  // too many (MI355X_MICROARCH.md, residency): then one workgroup per CU less
  if (n_cu <= 0 || vgprs <= 0 || api_blocks_per_cu <= 0 || wg_threads <= 0) return 0;
  const int alloc = (vgprs + 7) / 8 * 8;
  const int per_simd = alloc > 512 ? 0 : std::min(8, 512 / alloc);
  const int wpb = (wg_threads + IA_WAVE - 1) / IA_WAVE;
  int per_cu = std::min(4 * per_simd, api_blocks_per_cu * wpb);
  if (per_simd > 3) per_cu = std::min(per_cu, (api_blocks_per_cu - 1) * wpb);
  if (per_cu <= 0) return 0;
  const int slots = per_cu * n_cu;
  return 2 * slots - (2 * slots) / 16;
}
int ia_chain_choice(int level_waves, int in_flight, int budget, int two_wave) {
  // what a level whose widest chained launch has level_waves one-wave workgroups takes of the
  // budget, in_flight of it reserved already: the two-wave form (option "gather_wave") reserves
  // twice its waves; refused that, the one-wave form its single reservation; refused that too,
  // the level runs unchained
  if (level_waves <= 0 || in_flight < 0 || budget <= 0) return 0;
  const int64_t left = (int64_t)budget - in_flight;
  if (two_wave && 2 * (int64_t)level_waves <= left) return 2;
  return level_waves <= left ? 1 : 0;
}

}  // extern "C"
