// ia_comm.cpp — how the ranks of a sharded level reach each other: the RCCL communicator, the
// uncached peer-write exchange buffer and its IPC mappings, and the pure helpers that say which
// DB tiles a rank scans and how per-shard winners merge.
#include <rccl/rccl.h>

#include <cstring>

#include "ia_host.h"

namespace ia_host {

bool shard_level(int64_t n_tiles, int world) { return world > 1 && n_tiles >= 64 * (int64_t)world; }

void comm_close(ia_ctx *c) {
  if (c->comm) ncclCommDestroy(c->comm);
  for (int p = 0; p < IA_XCHG_MAXW; p++)
    if (c->xmapped[p]) hipIpcCloseMemHandle(c->xpeer[p]);
}

// fresh = true (ia_xchg_alloc, before the ranks swap handles): a reused buffer is zeroed too and
// the sequence restarts, so no seq word left from an earlier exchange (or an emulated run on this
// context) can match the restarted sequence; the handle swap orders every rank's zeroing before
// any peer's first store
int xchg_alloc(ia_ctx *c, int world, bool fresh) {
  const size_t bytes = ia_xslots_bytes(world) + 2 * XOLayout::PARITY;
  if (c->xbuf && c->xbuf_w >= world) {
    if (fresh) {
      HIP_TRY(hipStreamSynchronize(c->st));
      HIP_TRY(hipMemset(c->xbuf, 0, ia_xslots_bytes(c->xbuf_w) + 2 * XOLayout::PARITY));
      HIP_TRY(hipDeviceSynchronize());
      c->xbuf_w = world;
      c->xseq = 0;
      c->xfresh = true;
    }
    return IA_OK;
  }
  if (c->xbuf) hipFree(c->xbuf);
  c->xbuf = nullptr;
  // winner slots (exchange = 1) + two parities of the owner-computes area (exchange = 2)
  // uncached: peers' xGMI stores and this device's polling loads meet in memory, not in an L2
  HIP_TRY(hipExtMallocWithFlags(&c->xbuf, bytes, hipDeviceMallocUncached));
  HIP_TRY(hipMemset(c->xbuf, 0, bytes));
  HIP_TRY(hipDeviceSynchronize());
  c->xbuf_w = world;
  c->xseq = 0;
  c->xfresh = fresh;
  int rc;
  if ((rc = c->xerr.ensure(4))) return rc;
  return IA_OK;
}

}  // namespace ia_host

using namespace ia_host;

extern "C" {

int ia_comm_unique_id(unsigned char id_out[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  std::memcpy(id_out, &id, 128);
  return IA_OK;
}

int ia_comm_init(ia_ctx *c, int rank, int world, const unsigned char id[128]) {
  if (!c || world < 1 || rank < 0 || rank >= world) return fail(IA_EINVAL, "ia_comm_init: bad rank/world");
  HIP_TRY(hipSetDevice(c->dev));
  if (c->comm) ncclCommDestroy(c->comm);
  c->comm = nullptr;
  // the RCCL all-gather replaces any peer-write exchange opened before (ia_xchg_open)
  for (int p = 0; p < IA_XCHG_MAXW; p++) {
    if (c->xmapped[p]) hipIpcCloseMemHandle(c->xpeer[p]);
    c->xmapped[p] = false;
    c->xpeer[p] = nullptr;
  }
  c->exchange = 0;
  c->rank = rank;
  c->world = world;
  if (world == 1) return IA_OK;
  ncclUniqueId uid;
  std::memcpy(&uid, id, 128);
  NCCL_TRY(ncclCommInitRank(&c->comm, world, uid, rank));
  return IA_OK;
}

int ia_xchg_alloc(ia_ctx *c, int world, unsigned char handle_out[64]) {
  if (!c || !handle_out || world < 1 || world > IA_XCHG_MAXW) return fail(IA_EINVAL, "ia_xchg_alloc: world must be 1..16");
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t size");
  HIP_TRY(hipSetDevice(c->dev));
  int rc;
  if ((rc = xchg_alloc(c, world, true))) return rc;
  hipIpcMemHandle_t h;
  HIP_TRY(hipIpcGetMemHandle(&h, c->xbuf));
  std::memcpy(handle_out, &h, 64);
  return IA_OK;
}

int ia_xchg_open(ia_ctx *c, int rank, int world, const unsigned char *handles) {
  if (!c || !handles || world < 1 || world > IA_XCHG_MAXW || rank < 0 || rank >= world)
    return fail(IA_EINVAL, "ia_xchg_open: bad rank / world");
  if (!c->xbuf || c->xbuf_w != world || !c->xfresh)
    return fail(IA_EINVAL, "ia_xchg_open: call ia_xchg_alloc with this world first (once per ia_xchg_open)");
  HIP_TRY(hipSetDevice(c->dev));
  for (int p = 0; p < IA_XCHG_MAXW; p++)
    if (c->xmapped[p]) {
      hipIpcCloseMemHandle(c->xpeer[p]);
      c->xmapped[p] = false;
    }
  for (int p = 0; p < world; p++) {
    if (p == rank) {
      c->xpeer[p] = (XSlot *)c->xbuf;
      continue;
    }
    hipIpcMemHandle_t h;
    std::memcpy(&h, handles + (size_t)64 * p, 64);
    void *ptr = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
    c->xpeer[p] = (XSlot *)ptr;
    c->xmapped[p] = true;
  }
  if (c->comm) ncclCommDestroy(c->comm);
  c->comm = nullptr;
  c->rank = rank;
  c->world = world;
  if (c->exchange == 0) c->exchange = 1;  // keep 2 (owner computes) when it was chosen before
  c->xseq = 0;  // the buffer was zeroed by ia_xchg_alloc: no stale seq word matches the new sequence
  c->xfresh = false;
  return IA_OK;
}

int ia_shard_tiles(int64_t n_rows, int world, int rank, int64_t *tile0, int64_t *tile1) {
  if (n_rows < 1 || world < 1 || rank < 0 || rank >= world || !tile0 || !tile1)
    return fail(IA_EINVAL, "ia_shard_tiles: bad args");
  const int64_t n_tiles = (n_rows + IA_TILE - 1) / IA_TILE;
  if (!shard_level(n_tiles, world)) {
    *tile0 = 0;
    *tile1 = n_tiles;
    return IA_OK;
  }
  *tile0 = n_tiles * rank / world;
  *tile1 = n_tiles * (rank + 1) / world;
  return IA_OK;
}

int ia_shard_tiles_pruned(int64_t n_rows, int world, int rank, int64_t *tile0, int64_t *tile1) {
  if (n_rows < 1 || world < 1 || rank < 0 || rank >= world || !tile0 || !tile1)
    return fail(IA_EINVAL, "ia_shard_tiles_pruned: bad args");
  const int64_t n_tiles = (n_rows + IA_TILE - 1) / IA_TILE;
  if (!shard_level(n_tiles, world)) {
    *tile0 = 0;
    *tile1 = n_tiles;
    return IA_OK;
  }
  *tile0 = ia_shard_off(n_tiles, world, rank);
  *tile1 = ia_shard_off(n_tiles, world, rank + 1);
  return IA_OK;
}

int64_t ia_shard_morton_tile(int64_t storage_tile, int64_t n_tiles, int world) {
  if (world < 1 || n_tiles < 1 || storage_tile < 0 || storage_tile >= n_tiles) return -1;
  return world > 1 ? ia_shard_morton_tile_(storage_tile, n_tiles, world) : storage_tile;
}

int ia_merge_winners(const double *dist, const int64_t *row, int world, int64_t nq, double *dist_out,
                     int64_t *row_out) {
  if (!dist || !row || !dist_out || !row_out || world < 1 || nq < 0) return fail(IA_EINVAL, "ia_merge_winners: bad args");
  for (int64_t m = 0; m < nq; m++) {
    double bd = dist[m];
    int64_t bi = row[m];
    for (int k = 1; k < world; k++) {  // identical order on every rank (k_finish_level)
      const double d = dist[(int64_t)k * nq + m];
      const int64_t i = row[(int64_t)k * nq + m];
      if (d < bd || (d == bd && i < bi)) {
        bd = d;
        bi = i;
      }
    }
    dist_out[m] = bd;
    row_out[m] = bi;
  }
  return IA_OK;
}

}  // extern "C"
