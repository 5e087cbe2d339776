// The knocked trunk kernels' body (knock_trunk.h): statements, included inside a kernel -- no include guard, no namespace.  Reads ka,
// tk and steps from the kernel around it.
    const IplanAcTraceArgs& a = tk.base;
    const int net = (int)blockIdx.y, which = trace_which(a);
    const IplanAcNet& nw = which ? a.critic : a.actor;
    const float* __restrict__ P = nw.params + (int64_t)net * nw.params_s_net;
    const IplanAcFeatures& ft = a.feat;
    const int l = lane_id(), w = uniform_i(wave_id()), n = l & 15, g = l >> 4;
    const int JT = (int)ko_trace_tiles(tk);
    const int64_t rows = (int64_t)a.E * steps;                               // the rows with a tile of their own
    const int64_t tile = (int64_t)blockIdx.x * TRUNK_WAVES + w;
    if (tile >= rows * JT) return;                                           // (whole wave; the kernels have no barrier)
    const KnockTile col = knock_tile(ka, ft, tile, JT, steps, net, n);       // (ac_kmap_ko.h)
    const bool valid = col.valid;
    const int64_t ec = col.ec, sc = col.sc;
    const int jt = col.jt;
    const KMap km = make_kmap(ft);                                           // (kfeat_ko reads the one-hot widths from it)
    const SalMap sm = sal_make_map(ft);                                      // (the K map as scalars: sal_body.h)
    const int F = sm.NW + ft.n_actions + ft.n_id, KT = sm.KT;

#include "trace_trunk_impl.h"
