// ia_level_owner.cpp — the owner-computes steps of a level (exchange = 2, ia_internal.h XOLayout;
// called from LevelRun::step in ia_level_run.cpp): the layout of a step, the exchange areas of its
// sequence number, and each owner's gather (+ publish or K2s), this process's shard scans and
// each owner's merge (+ the next step's gather).
#include "ia_level_run.h"

namespace ia_host {

// parity base of rank p's area for the step of sequence seq (emulated: one area serves every shard)
char *LevelRun::xo_area(int p, unsigned seq) const {
  return (char *)(P.sharded ? (void *)c->xpeer[p] : c->xbuf) + ia_xslots_bytes(P.Wsh) + (size_t)(seq & 1u) * XOLayout::PARITY;
}
// the areas of the first n ranks
void LevelRun::xo_areas(char *(&area)[IA_XCHG_MAXW], int n, unsigned seq) const {
  for (int p = 0; p < n; p++) area[p] = xo_area(p, seq);
}
// what local owner jl's gather publishes into: every rank's area, from the owner's first slot
XOPub LevelRun::owner_pub(int jl, int Mpj, unsigned seq) const {
  XOPub xp{};
  xp.W = P.sharded ? P.Wsh : 1;
  xo_areas(xp.area, xp.W, seq);
  xp.slot0 = owner_of(jl) * Mpj;
  xp.seq = seq;
  return xp;
}

OwnerLayout LevelRun::owner_layout(int M) const {
  OwnerLayout l;
  l.Mpj = (int)tile_pad(M);
  l.ink = l.Mpj <= ia_k3h_qtmax(g.KS) * IA_TILE && !c->xo_presort;
  l.QTs = l.ink ? l.Mpj / IA_TILE : P.xo_QTs;
  l.Mrec = P.Wsh * l.QTs * IA_TILE;
  l.nqb = l.ink ? P.Wsh : P.Wsh * P.xo_bpj;
  // one chunk count for every shard (the owners' merges index records as shard * nch + chunk
  // and map a chunk back to its tiles with it): from the smallest shard, which every rank
  // computes alike (shards differ by at most one tile, ia_shard_off)
  l.nch = scan_chunks((int)(g.n_tiles / P.Wsh), l.nqb);
  return l;
}

OwnerStep LevelRun::owner_step(const StepDesc &sd) {
  OwnerStep os;
  static_cast<OwnerLayout &>(os) = owner_layout(sd.M);
  os.seq = ++c->xseq;
  os.loc = xo_area(P.sharded ? c->rank : 0, os.seq);
  os.s1 = step_desc(g, sd.t, 1);
  return os;
}

// the level's part of an owner's merge arguments: the whole level's table and boxes, the exchange
void LevelRun::init_owner_merge_args() {
  mxo = ma;
  mxo.rr = 1;
  mxo.NT = g.n_tiles;
  mxo.boxes = c->boxes.as<float4>();
  mxo.pos2row = g.pos2row;
  mxo.xo_inv = c->xo_inv.as<int>();
  mxo.xo_W = P.Wsh;
  mxo.xo_err = c->xerr.as<unsigned>();
  mxo.xo_timeout = IA_WAIT_TICKS;
}

// owner jl's K2s: its queries sorted into every rank's area
void LevelRun::owner_sort(const StepDesc &sd, const OwnerStep &os, const QBufs &q, int jl) {
  const size_t q0 = (size_t)jl * os.Mpj;
  XOSort xs{};
  xs.inv = c->xo_inv.as<int>();
  xs.W = P.sharded ? P.Wsh : 1;
  xo_areas(xs.area, xs.W, os.seq);
  xs.q0 = 0;
  xs.Mj = sd.M;
  xs.tile0 = owner_of(jl) * os.QTs;
  xs.QTs = os.QTs;
  xs.seq = os.seq;
  ia_launch_query_sort_xo(q.qinfo + 3 * q0, (char *)c->qf.p + q0 * P.db_row_bytes, xs, c->st);
}

void LevelRun::owner_gather(const StepDesc &sd, const OwnerStep &os, const QBufs &q) {
  for (int jl = 0; jl < P.J; jl++) {
    const size_t q0 = (size_t)jl * os.Mpj;
    if (!(chain && gathered == sd.t)) {  // else K2p (+ publish) ran in the previous step's fused merge
      const XOPub xp = os.ink ? owner_pub(jl, os.Mpj, os.seq) : XOPub{};
      ia_launch_gather_p(g, os.s1, in.Bim, in.job(jl), c->mu.as<double>(), q.q64 + q0 * g.D, q.qn2 + q0,
                         (char *)c->qf.p + q0 * P.db_row_bytes, c->db64.as<double>(), c->pr_basis.as<double>(), ufac,
                         q.qinfo + 3 * q0, in.Aim, c->st, &xp);
    }
    if (!os.ink) owner_sort(sd, os, q, jl);
  }
}

int LevelRun::owner_scan(const StepDesc &sd, const OwnerStep &os) {
  const int Wsh = P.Wsh;
  tally.begin_step(sd.t);
  for (size_t i = 0; i < P.shards.size(); i++) {
    const int n = P.shards[i].t1 - P.shards[i].t0;
    if ((n + os.nch - 1) / os.nch > IA_K3P_MAXK_LDS || (int64_t)Wsh * os.nch * os.Mrec > IA_XO_MAXREC)
      return fail(IA_EINVAL, "ia_synthesize_level: exchange = 2: shard too large for the pruned scan's chunks");
    XOScan xs{};
    xo_areas(xs.area, Wsh, os.seq);
    xs.flag = reinterpret_cast<const unsigned *>(os.loc + (os.ink ? XOLayout::QSEQ : XOLayout::FLAG));
    xs.inv = c->xo_inv.as<int>();
    xs.on = 1;
    xs.s = P.sharded ? c->rank : (int)i;
    xs.bpj = os.ink ? 1 : P.xo_bpj;
    xs.Mrec = os.Mrec;
    xs.seq = os.seq;
    xs.err = c->xerr.as<unsigned>();
    xs.timeout_ticks = IA_WAIT_TICKS;
    K3pLaunch k = scan_base(i, sd);  // the queries come from this process's area, the records go to the owners'
    k.qf = os.loc + XOLayout::FRAG;
    k.qinfo = reinterpret_cast<const float4 *>(os.loc + XOLayout::INFO);
    k.order = reinterpret_cast<const int *>(os.loc + XOLayout::ORD);
    k.tbox = reinterpret_cast<const float4 *>(os.loc + XOLayout::TBOX);
    k.qt = os.ink ? os.QTs : P.xo_QTx;
    k.M = sd.M;
    k.Mpad = os.ink ? os.Mpj : os.Mrec;
    k.nwg = os.nch;
    k.nqb = os.nqb;
    k.qt_end = Wsh * os.QTs;
    k.xo = &xs;
    int rc;
    if ((rc = launch_scan(k, !os.ink))) return rc;
    tally.add((double)n * Wsh * os.QTs, (double)n * os.nqb, 0., true,
              scan_fixed_bytes((double)n * os.nqb, os.Mrec, (double)os.Mrec * os.nch * 24), (double)n * P.tile_bytes);
  }
  tally.end_step();
  return IA_OK;
}

int LevelRun::owner_merge(const StepDesc &sd, const OwnerStep &os, const QBufs &q) {
  const int64_t t = sd.t;
  const int Wsh = P.Wsh;
  // the next step's layout (fused merge + gather: each owner publishes its next queries)
  const bool fuse_next = fuses_next(t);
  StepDesc sn{};
  OwnerLayout ln{};
  if (fuse_next) {
    int rc;
    if ((rc = link.wait_dep(t + 1))) return rc;
    sn = step_desc(g, t + 1, 1);
    ln = owner_layout(sn.M);
  }
  for (int jl = 0; jl < P.J; jl++) {
    const size_t q0 = (size_t)jl * os.Mpj;
    MergeArgs mx = mxo;
    mx.q64 = q.q64 + q0 * g.D;
    mx.qn2 = q.qn2 + q0;
    mx.qinfo = q.qinfo + 3 * q0;
    mx.rec = reinterpret_cast<const float4 *>(os.loc + XOLayout::REC);
    mx.xo_rts = reinterpret_cast<const unsigned long long *>(os.loc + XOLayout::RTS);
    mx.nwg = Wsh * os.nch;
    mx.xo_nch = os.nch;
    mx.xo_Mrec = os.Mrec;
    mx.xo_o0 = owner_of(jl);
    mx.xo_M = sd.M;
    mx.xo_QTs = os.QTs;
    mx.xo_seq = os.seq;
    mx.stamp = stamps.mg();
    if (!fuse_next) {
      ia_launch_merge(g, os.s1, in.Aim, mx, c->win.as<Winner>(), in.job(jl), true, c->st);
      continue;
    }
    NextStep nx = next_step(sn, jl, (size_t)jl * ln.Mpj);
    if (ln.ink) {  // the next step's queries go straight to every rank's area (else its K2s sorts them)
      nx.xp = owner_pub(jl, ln.Mpj, os.seq + 1);
      if (P.sharded && c->xo_wait && jl == P.J - 1) {  // ranks: wait here for every owner's next queries
        nx.wait_seq = reinterpret_cast<const unsigned *>(xo_area(c->rank, os.seq + 1) + XOLayout::QSEQ);
        nx.wait_n = Wsh * ln.Mpj;
      }
    }
    ia_launch_merge_gather(g, os.s1, in.Aim, mx, in.job(jl), in.Bim, nx, true, c->st);
  }
  if (fuse_next) gathered = t + 1;
  return IA_OK;
}

}  // namespace ia_host
