// somar_amd/csrc/level.cpp -- layout tables, HBM allocation, ghost-exchange plan.
#include "level.h"
#include "march_plan.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>

namespace somar {

bool coarsenable(const std::vector<IBox>& boxes, const int* r)
{
    // Chombo: refine(coarsen(b, r), r) == b for every box
    for (const IBox& b : boxes)
        if (!(b.coarsen(r).refine(r) == b)) return false;
    return true;
}

// Pure host logic (no GPU): the ghost-exchange plan of rank `myrank` for the layout -- Chombo's
// Copier(grids, grids, domain, ghost, exchange=true).  Items carry GLOBAL box indices in
// src_patch/dst_patch.  Both sides of a rank pair enumerate (dst box, src box, periodic shift) in the
// same order, so the i-th item of a send message is the i-th item of the matching receive message.
ExchangePlan build_exchange_plan(const IBox& domain, const bool periodic[3], const int ghost[3],
                                 const std::vector<IBox>& boxes, const std::vector<int>& owner, int myrank)
{
    ExchangePlan plan;
    std::vector<std::array<int, 3>> shifts;
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int cc = -1; cc <= 1; ++cc) {
                if ((a && !periodic[0]) || (b && !periodic[1]) || (cc && !periodic[2])) continue;
                shifts.push_back({a * domain.size(0), b * domain.size(1), cc * domain.size(2)});
            }
    struct Remote { int peer; CopyItem it; };
    std::vector<Remote> sends, recvs;
    for (size_t di = 0; di < boxes.size(); ++di) {
        const IBox gbox = boxes[di].grow(ghost);
        for (size_t si = 0; si < boxes.size(); ++si) {
            const bool dl = owner[di] == myrank, sl = owner[si] == myrank;
            if (!dl && !sl) continue;
            for (const auto& sh : shifts) {
                if (si == di && sh[0] == 0 && sh[1] == 0 && sh[2] == 0) continue;
                const IBox img = boxes[si].shift(sh.data());
                const IBox r = gbox & img;
                if (r.empty()) continue;
                CopyItem it;
                std::memset(&it, 0, sizeof(it));
                it.src_patch = (int)si;
                it.dst_patch = (int)di;
                for (int d = 0; d < 3; ++d) {
                    it.n[d] = r.size(d);
                    it.dst_lo[d] = r.lo[d] - boxes[di].lo[d];
                    it.src_lo[d] = r.lo[d] - sh[d] - boxes[si].lo[d];
                }
                if (dl && sl) plan.local.push_back(it);
                else if (sl) sends.push_back({owner[di], it});
                else recvs.push_back({owner[si], it});
            }
        }
    }
    for (auto& r : sends) plan.peers.push_back(r.peer);
    for (auto& r : recvs) plan.peers.push_back(r.peer);
    std::sort(plan.peers.begin(), plan.peers.end());
    plan.peers.erase(std::unique(plan.peers.begin(), plan.peers.end()), plan.peers.end());
    for (int q : plan.peers) {
        plan.soff.push_back(plan.send_total);
        for (auto& r : sends)
            if (r.peer == q) {
                plan.send_items.push_back(r.it);
                plan.send_itemoff.push_back(plan.send_total);
                plan.send_total += (long long)r.it.n[0] * r.it.n[1] * r.it.n[2];
            }
        plan.scount.push_back(plan.send_total - plan.soff.back());
        plan.roff.push_back(plan.recv_total);
        for (auto& r : recvs)
            if (r.peer == q) {
                plan.recv_items.push_back(r.it);
                plan.recv_itemoff.push_back(plan.recv_total);
                plan.recv_total += (long long)r.it.n[0] * r.it.n[1] * r.it.n[2];
            }
        plan.rcount.push_back(plan.recv_total - plan.roff.back());
    }
    return plan;
}

// a minus b as a list of disjoint boxes (at most 6)
void box_subtract(const IBox& a, const IBox& b, std::vector<IBox>& out)
{
    const IBox c = a & b;
    if (c.empty()) { out.push_back(a); return; }
    IBox rest = a;
    for (int d = 2; d >= 0; --d) {
        if (rest.lo[d] < c.lo[d]) { IBox p = rest; p.hi[d] = c.lo[d] - 1; out.push_back(p); rest.lo[d] = c.lo[d]; }
        if (rest.hi[d] > c.hi[d]) { IBox p = rest; p.lo[d] = c.hi[d] + 1; out.push_back(p); rest.hi[d] = c.hi[d]; }
    }
}

std::vector<std::array<int, 3>> periodic_shifts(const IBox& domain, const bool periodic[3])
{
    // the unshifted image first, then the others in (x, y, z) lexicographic order of (-n, 0, +n)
    std::vector<std::array<int, 3>> shifts;
    shifts.push_back({0, 0, 0});
    for (int a = -1; a <= 1; ++a)
        for (int b = -1; b <= 1; ++b)
            for (int cc = -1; cc <= 1; ++cc) {
                if ((a && !periodic[0]) || (b && !periodic[1]) || (cc && !periodic[2])) continue;
                if (!a && !b && !cc) continue;
                shifts.push_back({a * domain.size(0), b * domain.size(1), cc * domain.size(2)});
            }
    return shifts;
}

// `region` minus every box of `boxes` and every periodic image of them
std::vector<IBox> uncovered(const IBox& region, const std::vector<IBox>& boxes, const IBox& domain,
                            const bool periodic[3])
{
    std::vector<IBox> cur{region};
    const auto shifts = periodic_shifts(domain, periodic);
    for (const IBox& b : boxes)
        for (const auto& sh : shifts) {
            const IBox img = b.shift(sh.data());
            if ((img & region).empty()) continue;
            std::vector<IBox> nxt;
            for (const IBox& c : cur) box_subtract(c, img, nxt);
            cur.swap(nxt);
            if (cur.empty()) return cur;
        }
    return cur;
}

static bool contains_cell(const IBox& b, const int c[3])
{
    for (int d = 0; d < 3; ++d)
        if (c[d] < b.lo[d] || c[d] > b.hi[d]) return false;
    return true;
}

// CFRegion of this level + homogeneousCFInterp weights (HomogeneousCFInterp.cpp:56, 72-73)
void Level::define_cf(const double dxCrse[3])
{
    hcf.clear();
    int g[3];
    for (int d = 0; d < 3; ++d) g[d] = periodic[d] ? 1 : 0;
    const IBox dom = domain.grow(g);
    for (int pi = 0; pi < npatches(); ++pi) {
        const PatchDesc& p = hpatches[pi];
        const IBox valid = boxes[local[pi]];
        const long long st[3] = {1, p.pj, p.pk};
        for (int d = 0; d < 3; ++d) {
            if (!active[d]) continue;
            for (int s = 0; s < 2; ++s) {
                IBox gb = valid;
                if (s == 0) { gb.lo[d] = valid.lo[d] - 1; gb.hi[d] = valid.lo[d] - 1; }
                else { gb.lo[d] = valid.hi[d] + 1; gb.hi[d] = valid.hi[d] + 1; }
                gb = gb & dom;
                if (gb.empty()) continue;
                for (const IBox& u : uncovered(gb, boxes, domain, periodic))
                    for (int k = u.lo[2]; k <= u.hi[2]; ++k)
                        for (int j = u.lo[1]; j <= u.hi[1]; ++j)
                            for (int i = u.lo[0]; i <= u.hi[0]; ++i) {
                                CFCell c;
                                c.off = p.off + (i - p.lo[0]) + st[1] * (j - p.lo[1]) + st[2] * (k - p.lo[2]);
                                c.stride = (int)(s ? st[d] : -st[d]);
                                c.dir = d | (p.n[d] == 1 ? 4 : 0);
                                hcf.push_back(c);
                            }
            }
        }
    }
    d_cf = DevBuf<CFCell>::from(hcf);
    ncf = (int)hcf.size();
    for (int d = 0; d < 3; ++d) {
        const double Df = dx[d], Dc = dxCrse[d];
        cf_c1[d] = 2.0 * (Dc - Df) / (Dc + Df);
        cf_c2[d] = -(Dc - Df) / (Dc + 3.0 * Df);
        cf_fac[d] = 1.0 - 2.0 * Df / (Df + Dc);
    }

    // ---- what the fused sweep needs (see level.h) ----------------------------------------------------
    cf_fusable = true;
    hcfx = hcf;
    const auto shifts = periodic_shifts(domain, periodic);
    std::vector<IBox> near;  // box images around the patch at hand
    auto covered1 = [&](const int c[3]) {
        for (const IBox& b : near)
            if (contains_cell(b, c)) return true;
        return false;
    };
    for (int pi = 0; pi < npatches(); ++pi) {
        PatchDesc& p = hpatches[pi];
        const IBox valid = boxes[local[pi]];
        const long long st[3] = {1, p.pj, p.pk};
        p.cf = 0;
        near.clear();
        {
            const int g2[3] = {2, 2, 2};
            const IBox around = valid.grow(g2);
            for (const IBox& b : boxes)
                for (const auto& sh : shifts) {
                    const IBox img = b.shift(sh.data());
                    if (!(img & around).empty()) near.push_back(img);
                }
        }
        for (int d = 0; d < 3; ++d) {
            if (!active[d]) continue;
            for (int s = 0; s < 2; ++s) {
                IBox gb = valid;
                if (s == 0) { gb.lo[d] = gb.hi[d] = valid.lo[d] - 1; }
                else { gb.lo[d] = gb.hi[d] = valid.hi[d] + 1; }
                gb = gb & dom;
                if (gb.empty()) continue;
                long long nunc = 0;
                for (const IBox& u : uncovered(gb, boxes, domain, periodic)) nunc += u.numPts();
                if (nunc == gb.numPts()) p.cf |= 1 << (2 * d + s);
                else if (nunc != 0) cf_fusable = false;  // a face that is only partly coarse-fine
                if (nunc != 0 && p.n[d] < 2) cf_fusable = false;
            }
        }
        // edge ghosts: two coordinates one cell outside the box
        for (int d1 = 0; d1 < 3 && cf_fusable; ++d1)
            for (int d2 = d1 + 1; d2 < 3 && cf_fusable; ++d2) {
                if (!active[d1] || !active[d2]) continue;
                const int d3 = 3 - d1 - d2;
                for (int s1 = 0; s1 < 2; ++s1)
                    for (int s2 = 0; s2 < 2; ++s2)
                        for (int t = valid.lo[d3]; t <= valid.hi[d3] && cf_fusable; ++t) {
                            int g[3];
                            g[d1] = s1 ? valid.hi[d1] + 1 : valid.lo[d1] - 1;
                            g[d2] = s2 ? valid.hi[d2] + 1 : valid.lo[d2] - 1;
                            g[d3] = t;
                            if (!contains_cell(dom, g) || covered1(g)) continue;
                            // candidates: directions along which the cell next to g (towards the box) is a real
                            // cell of a neighbouring box, which then owns g as one of ITS face ghosts
                            int ncand = 0, cd = -1, cs = 0;
                            const int dd[2] = {d1, d2}, ss[2] = {s1, s2};
                            for (int q = 0; q < 2; ++q) {
                                int h[3] = {g[0], g[1], g[2]};
                                h[dd[q]] += ss[q] ? -1 : 1;
                                if (!covered1(h)) continue;
                                int h2[3] = {h[0], h[1], h[2]};
                                h2[dd[q]] += ss[q] ? -1 : 1;
                                if (!covered1(h2)) { cf_fusable = false; break; }  // neighbour box one cell wide
                                ++ncand;
                                cd = dd[q];
                                cs = ss[q];
                            }
                            if (ncand == 2) cf_fusable = false;  // re-entrant corner of the refined region
                            if (ncand != 1 || !cf_fusable) continue;
                            CFCell c;
                            c.off = p.off + (g[0] - p.lo[0]) + st[1] * (g[1] - p.lo[1]) + st[2] * (g[2] - p.lo[2]);
                            c.stride = (int)(cs ? st[cd] : -st[cd]);
                            c.dir = cd;
                            hcfx.push_back(c);
                        }
            }
    }
    if (!cf_fusable) hcfx = hcf;
    for (int d = 0; d < 3; ++d) {
        cf_faces[d].reset();
        if (active[d] && ((cf_fusable && ncf > 0) || (!periodic[d] && bc_type[d][1] == BC_DIRI))) {
            int gh[3];
            for (int e = 0; e < 3; ++e) gh[e] = active[e] ? FRAME : 0;
            cf_faces[d].reset(new Copier);
            cf_faces[d]->define_faces(domain, periodic, *this, d, gh, comm);
        }
    }
    d_cfx = DevBuf<CFCell>::from(hcfx);
    ncfx = (int)hcfx.size();
    d_patches = DevBuf<PatchDesc>::from(hpatches);  // the flag bits
    dev.patches = d_patches;
    refresh_params();
    SOMAR_HIP(hipDeviceSynchronize());
}

// ------------------------------------------------------------------------------------
// Copier between two layouts
// ------------------------------------------------------------------------------------
// Pure host logic.  Items carry GLOBAL box indices; every rank enumerates (dst box, src box, shift) in the
// same order, so the i-th item of a send message is the i-th item of the matching receive message.
namespace {
struct Remote { int peer; CopyItem it; };
// peers in ascending order, one message per peer: its items in walk order, offsets in doubles
void layout_messages(ExchangePlan& plan, const std::vector<Remote>& sends, const std::vector<Remote>& recvs)
{
    for (auto& r : sends) plan.peers.push_back(r.peer);
    for (auto& r : recvs) plan.peers.push_back(r.peer);
    std::sort(plan.peers.begin(), plan.peers.end());
    plan.peers.erase(std::unique(plan.peers.begin(), plan.peers.end()), plan.peers.end());
    for (int q : plan.peers) {
        plan.soff.push_back(plan.send_total);
        for (auto& r : sends)
            if (r.peer == q) {
                plan.send_items.push_back(r.it);
                plan.send_itemoff.push_back(plan.send_total);
                plan.send_total += (long long)r.it.n[0] * r.it.n[1] * r.it.n[2];
            }
        plan.scount.push_back(plan.send_total - plan.soff.back());
        plan.roff.push_back(plan.recv_total);
        for (auto& r : recvs)
            if (r.peer == q) {
                plan.recv_items.push_back(r.it);
                plan.recv_itemoff.push_back(plan.recv_total);
                plan.recv_total += (long long)r.it.n[0] * r.it.n[1] * r.it.n[2];
            }
        plan.rcount.push_back(plan.recv_total - plan.roff.back());
    }
}
}  // namespace

ExchangePlan build_copy_plan(const IBox& domain, const bool periodic[3], const std::vector<IBox>& srcBoxes,
                             const std::vector<int>& srcOwner, const std::vector<IBox>& dstBoxes,
                             const std::vector<int>& dstOwner, const int ghost[3], int myrank, bool ring_only)
{
    ExchangePlan plan;
    const auto shifts = periodic_shifts(domain, periodic);
    std::vector<Remote> sends, recvs;
    for (size_t di = 0; di < dstBoxes.size(); ++di) {
        const IBox gbox = dstBoxes[di].grow(ghost);
        for (size_t si = 0; si < srcBoxes.size(); ++si) {
            const bool dl = dstOwner[di] == myrank, sl = srcOwner[si] == myrank;
            if (!dl && !sl) continue;
            for (const auto& sh : shifts) {
                const IBox r0 = gbox & srcBoxes[si].shift(sh.data());
                if (r0.empty()) continue;
                // ring_only: the part of the region outside the destination box (its ghost ring), as up to six slabs in a fixed
                // order -- every rank derives the same pieces, so sends and receives still pair up
                std::vector<IBox> pieces;
                if (!ring_only) pieces.push_back(r0);
                else {
                    IBox rest = r0;
                    const IBox& V = dstBoxes[di];
                    for (int d = 2; d >= 0 && !rest.empty(); --d) {
                        IBox lo = rest, hi = rest;
                        lo.hi[d] = std::min(rest.hi[d], V.lo[d] - 1);
                        hi.lo[d] = std::max(rest.lo[d], V.hi[d] + 1);
                        if (!lo.empty()) pieces.push_back(lo);
                        if (!hi.empty()) pieces.push_back(hi);
                        rest.lo[d] = std::max(rest.lo[d], V.lo[d]);
                        rest.hi[d] = std::min(rest.hi[d], V.hi[d]);
                    }
                }
                for (const IBox& r : pieces) {
                    CopyItem it;
                    std::memset(&it, 0, sizeof(it));
                    it.src_patch = (int)si;
                    it.dst_patch = (int)di;
                    for (int d = 0; d < 3; ++d) {
                        it.n[d] = r.size(d);
                        it.dst_lo[d] = r.lo[d] - dstBoxes[di].lo[d];
                        it.src_lo[d] = r.lo[d] - sh[d] - srcBoxes[si].lo[d];
                    }
                    if (dl && sl) plan.local.push_back(it);
                    else if (sl) sends.push_back({dstOwner[di], it});
                    else recvs.push_back({srcOwner[si], it});
                }
            }
        }
    }
    layout_messages(plan, sends, recvs);
    return plan;
}

// Face-centred data of direction `dir` between two layouts.  For one destination box the candidate sources are walked from
// the LAST in priority order (periodic images after unshifted boxes, within each the layout order) to the first, and each
// takes only what no later one has taken: every destination face is written by exactly one item -- the later box wins --
// whatever order the items run in.
ExchangePlan build_face_copy_plan(const IBox& domain, const bool periodic[3], const std::vector<IBox>& srcBoxes,
                                  const std::vector<int>& srcOwner, const std::vector<IBox>& dstBoxes,
                                  const std::vector<int>& dstOwner, int dir, int myrank)
{
    ExchangePlan plan;
    const auto shifts = periodic_shifts(domain, periodic);   // the unshifted image first
    std::vector<Remote> sends, recvs;
    for (size_t di = 0; di < dstBoxes.size(); ++di) {
        IBox dface = dstBoxes[di];
        dface.hi[dir] += 1;
        std::vector<IBox> taken;
        for (size_t shi = shifts.size(); shi-- > 0;) {
            const auto& sh = shifts[shi];
            for (size_t si = srcBoxes.size(); si-- > 0;) {
                IBox sface = srcBoxes[si];
                sface.hi[dir] += 1;
                const IBox r0 = dface & sface.shift(sh.data());
                if (r0.empty()) continue;
                std::vector<IBox> pieces{r0};
                for (const IBox& t : taken) {
                    std::vector<IBox> nxt;
                    for (const IBox& c : pieces) box_subtract(c, t, nxt);
                    pieces.swap(nxt);
                }
                taken.push_back(r0);
                const bool dl = dstOwner[di] == myrank, sl = srcOwner[si] == myrank;
                if (!dl && !sl) continue;
                for (const IBox& r : pieces) {
                    CopyItem it;
                    std::memset(&it, 0, sizeof(it));
                    it.src_patch = (int)si;
                    it.dst_patch = (int)di;
                    for (int d = 0; d < 3; ++d) {
                        it.n[d] = r.size(d);
                        it.dst_lo[d] = r.lo[d] - dstBoxes[di].lo[d];
                        it.src_lo[d] = r.lo[d] - sh[d] - srcBoxes[si].lo[d];
                    }
                    if (dl && sl) plan.local.push_back(it);
                    else if (sl) sends.push_back({dstOwner[di], it});
                    else recvs.push_back({srcOwner[si], it});
                }
            }
        }
    }
    layout_messages(plan, sends, recvs);
    return plan;
}

void Copier::define_face_copy(const IBox& domain, const bool periodic[3], const Level& src, const Level& dst, int dir, Comm* comm)
{
    src_ = &src;
    dst_ = &dst;
    comm_ = comm;
    SOMAR_CHECK(dir >= 0 && dir < 3, "face copy: bad direction");
    plan = build_face_copy_plan(domain, periodic, src.boxes, src.owner, dst.boxes, dst.owner, dir, comm ? comm->rank : 0);
    std::vector<int> sp(src.boxes.size(), -1), dp(dst.boxes.size(), -1);
    for (int pi = 0; pi < (int)src.local.size(); ++pi) sp[src.local[pi]] = pi;
    for (int pi = 0; pi < (int)dst.local.size(); ++pi) dp[dst.local[pi]] = pi;
    for (CopyItem& it : plan.local) { it.src_patch = sp[it.src_patch]; it.dst_patch = dp[it.dst_patch]; }
    for (CopyItem& it : plan.send_items) it.src_patch = sp[it.src_patch];
    for (CopyItem& it : plan.recv_items) it.dst_patch = dp[it.dst_patch];
    upload_tables();
}

void Copier::define(const IBox& domain, const bool periodic[3], const Level& src, const Level& dst, const int ghost[3],
                    Comm* comm, bool ring_only)
{
    src_ = &src;
    dst_ = &dst;
    comm_ = comm;
    for (int d = 0; d < 3; ++d) SOMAR_CHECK(ghost[d] <= FRAME, "copier ghost wider than the device frame");
    plan = build_copy_plan(domain, periodic, src.boxes, src.owner, dst.boxes, dst.owner, ghost, comm ? comm->rank : 0, ring_only);
    std::vector<int> sp(src.boxes.size(), -1), dp(dst.boxes.size(), -1);
    for (int pi = 0; pi < (int)src.local.size(); ++pi) sp[src.local[pi]] = pi;
    for (int pi = 0; pi < (int)dst.local.size(); ++pi) dp[dst.local[pi]] = pi;
    for (CopyItem& it : plan.local) { it.src_patch = sp[it.src_patch]; it.dst_patch = dp[it.dst_patch]; }
    for (CopyItem& it : plan.send_items) it.src_patch = sp[it.src_patch];
    for (CopyItem& it : plan.recv_items) it.dst_patch = dp[it.dst_patch];
    upload_tables();
}

// Face-centred data of direction `dir`: the source of box b is faces(b, dir) -- the valid cells plus the layer
// that holds the box's HIGH face -- so a neighbour's frame also receives the coefficient of a face that no box
// owns as a low face (a box face on a coarse-fine boundary).  Run it BEFORE the ordinary exchange: where a real
// low-face owner exists its value then overwrites this one.
void Copier::define_faces(const IBox& domain, const bool periodic[3], const Level& L, int dir, const int ghost[3],
                          Comm* comm)
{
    src_ = &L;
    dst_ = &L;
    comm_ = comm;
    std::vector<IBox> fb = L.boxes;
    for (IBox& b : fb) b.hi[dir] += 1;
    plan = build_copy_plan(domain, periodic, fb, L.owner, L.boxes, L.owner, ghost, comm ? comm->rank : 0, false);
    std::vector<int> lp(L.boxes.size(), -1);
    for (int pi = 0; pi < (int)L.local.size(); ++pi) lp[L.local[pi]] = pi;
    for (CopyItem& it : plan.local) { it.src_patch = lp[it.src_patch]; it.dst_patch = lp[it.dst_patch]; }
    for (CopyItem& it : plan.send_items) it.src_patch = lp[it.src_patch];
    for (CopyItem& it : plan.recv_items) it.dst_patch = lp[it.dst_patch];
    // drop the copies of a box onto itself (same cells)
    std::vector<CopyItem> keep;
    for (const CopyItem& it : plan.local)
        if (!(it.src_patch == it.dst_patch && it.src_lo[0] == it.dst_lo[0] && it.src_lo[1] == it.dst_lo[1] &&
              it.src_lo[2] == it.dst_lo[2]))
            keep.push_back(it);
    plan.local.swap(keep);
    upload_tables();
}

void Copier::upload_tables()
{
    d_local = DevBuf<CopyItem>::from(plan.local);
    d_send = DevBuf<CopyItem>::from(plan.send_items);
    d_recv = DevBuf<CopyItem>::from(plan.recv_items);
    d_soff = DevBuf<long long>::from(plan.send_itemoff);
    d_roff = DevBuf<long long>::from(plan.recv_itemoff);
    d_sbuf = plan.send_total ? DevBuf<double>(plan.send_total) : DevBuf<double>();
    d_rbuf = plan.recv_total ? DevBuf<double>(plan.recv_total) : DevBuf<double>();
    SOMAR_HIP(hipDeviceSynchronize());
}

// Every rank ends up with every box: my boxes are copied locally and sent to every other rank, the others'
// boxes are received from their owners.  Both sides walk the boxes in layout order.
ExchangePlan build_allgather_plan(const std::vector<IBox>& boxes, const std::vector<int>& owner, int grow, int myrank,
                                  int nranks)
{
    ExchangePlan plan;
    auto item = [&](size_t b) {
        CopyItem it;
        std::memset(&it, 0, sizeof(it));
        it.src_patch = (int)b;
        it.dst_patch = (int)b;
        for (int d = 0; d < 3; ++d) {
            it.n[d] = boxes[b].size(d) + 2 * grow;
            it.src_lo[d] = -grow;
            it.dst_lo[d] = -grow;
        }
        return it;
    };
    for (size_t b = 0; b < boxes.size(); ++b)
        if (owner[b] == myrank) plan.local.push_back(item(b));
    for (int q = 0; q < nranks; ++q) {
        if (q == myrank) continue;
        plan.peers.push_back(q);
        plan.soff.push_back(plan.send_total);
        for (size_t b = 0; b < boxes.size(); ++b)
            if (owner[b] == myrank) {
                const CopyItem it = item(b);
                plan.send_items.push_back(it);
                plan.send_itemoff.push_back(plan.send_total);
                plan.send_total += (long long)it.n[0] * it.n[1] * it.n[2];
            }
        plan.scount.push_back(plan.send_total - plan.soff.back());
        plan.roff.push_back(plan.recv_total);
        for (size_t b = 0; b < boxes.size(); ++b)
            if (owner[b] == q) {
                const CopyItem it = item(b);
                plan.recv_items.push_back(it);
                plan.recv_itemoff.push_back(plan.recv_total);
                plan.recv_total += (long long)it.n[0] * it.n[1] * it.n[2];
            }
        plan.rcount.push_back(plan.recv_total - plan.roff.back());
    }
    return plan;
}

void Copier::define_allgather(const Level& src, const Level& dst, int grow, Comm* comm)
{
    src_ = &src;
    dst_ = &dst;
    comm_ = comm;
    SOMAR_CHECK(grow >= 0 && grow <= FRAME, "allgather: ghost wider than the device frame");
    SOMAR_CHECK(dst.boxes.size() == src.boxes.size() && dst.local.size() == dst.boxes.size(),
                "allgather: the destination layout must hold every box locally");
    plan = build_allgather_plan(src.boxes, src.owner, grow, comm ? comm->rank : 0, comm ? comm->size : 1);
    std::vector<int> sp(src.boxes.size(), -1);
    for (int pi = 0; pi < (int)src.local.size(); ++pi) sp[src.local[pi]] = pi;
    for (CopyItem& it : plan.local) it.src_patch = sp[it.src_patch];   // dst patch index = global box index
    for (CopyItem& it : plan.send_items) it.src_patch = sp[it.src_patch];
    upload_tables();
}

void Copier::run(const double* s, double* d, hipStream_t st) const
{
    const bool remote = !plan.peers.empty();
    if (remote) {
        launch_pack(st, src_->dev, d_send, d_soff, (int)plan.send_items.size(), const_cast<double*>(s), d_sbuf, true);
        comm_->neighbor_exchange(d_sbuf, d_rbuf, plan.peers, plan.soff, plan.scount, plan.roff, plan.rcount, st);
    }
    launch_copy_items2(st, src_->dev.patches, dst_->dev.patches, d_local, (int)plan.local.size(), s, d);
    if (remote) launch_pack(st, dst_->dev, d_recv, d_roff, (int)plan.recv_items.size(), d, d_rbuf, false);
}

// Tile tables of the k-marching kernels (fused 7-point sweep, 7-point operator / residual, 19-point kernels) and, on a sharded
// level, their split into tiles that read no remote ghost cell and the rest; march_plan.h builds them.  narrow7: the 7-point
// tables use the narrow lane classes for remainder columns.  That pays where the kernels are latency-bound -- a uniform metric,
// two or three streams (C4: 158 -> 112 ms per AMR V-cycle, c2_cartesian 134 -> 159 V-cycles/s) -- and costs where six streams
// are HBM-bound (512^3 stretched: residual 1.52 -> 2.00 ms: 64-byte row segments of six arrays), so PressureSolver::finalize asks
// for it on the depths whose metric it found uniform; the 19-point tables always use the classes.  tall7: finalize found the
// metric not uniform: the fused sweep's table takes tall tiles (march_plan.h) where the boxes are wide enough.
void Level::build_march_tiles(const MarchRequest& req)
{
    namespace mp = march_plan;
    march = req;
    ftiles.clear(); rtiles.clear(); qtiles.clear(); gtiles.clear(); stiles.clear();
    std::vector<mp::BoxSize> sizes;
    for (const PatchDesc& p : hpatches) sizes.push_back({p.n[0], p.n[1], p.n[2]});
    // Tuning::no_narrow_tiles, no_balanced_tiles: columns of equal width, all class 0 / plain 124-wide columns
    auto tuned = [&](mp::Shape s) {
        s.classes = s.classes && !tune.no_narrow_tiles;
        s.balanced = !tune.no_balanced_tiles;
        return s;
    };
    // tall tiles: the caller asks for them where the fused sweep can run at all (7-point operator, three active directions);
    // march_plan.h's rule sees the boxes, the kernel family and the metric flag; the switches that restore the equal columns
    // turn them off
    const bool tall = req.tall7 && !tune.no_narrow_tiles && tune.narrow_7pt != 0 &&
                      mp::tall_eligible(sizes, dev.fused_rows, dev.P.uniform != 0);
    const mp::Shape fshape = tuned(mp::fused_shape(dev.fused_rows, req.narrow7)), rshape = tuned(mp::resid_shape(req.narrow7));
    mp::Table f = mp::march_tiles(fshape, sizes, tall), r = mp::march_tiles(rshape, sizes);
    mp::number_slots(r.tiles);
    mp::Table q = mp::march_tiles(tuned(mp::full_shape(dev.full_rows)), sizes);
    if (!plan.peers.empty()) {
        // which marching tiles read a ghost cell that arrives from another rank?  The fused sweep reads phi two cells around
        // its columns and planes (the recomputed red ring) -- FRAME deep, as deep as the exchange fills; the operator one cell.
        std::vector<mp::Region> recv;
        for (const CopyItem& it : plan.recv_items)
            recv.push_back({it.dst_patch, {it.dst_lo[0], it.dst_lo[1], it.dst_lo[2]}, {it.n[0], it.n[1], it.n[2]}});
        auto split = [&](SplitTileTable& t, const mp::Table& all, const mp::Shape& shape, int halo) {
            std::vector<Tile> own, rem;
            mp::split(all.tiles, shape, halo, sizes, recv, own, rem);
            t.own.assign(std::move(own), all.classes);
            t.rem.assign(std::move(rem), all.classes);
        };
        split(ftiles, f, fshape, FRAME);
        split(rtiles, r, rshape, 1);
    }
    ftiles.all.assign(std::move(f.tiles), f.classes);
    rtiles.all.assign(std::move(r.tiles), r.classes);
    qtiles.assign(std::move(q.tiles), q.classes);
    if (req.fused19) {
        mp::Table g = mp::march_tiles(tuned(mp::fused19_shape()), sizes), sh = mp::shell_tiles(sizes);
        gtiles.assign(std::move(g.tiles), g.classes);
        stiles.assign(std::move(sh.tiles), sh.classes);
    }
}

void Level::define(const IBox& dom, const bool per[3], const double dx_[3], const int bct[3][2],
                   const std::vector<IBox>& bx, const std::vector<int>& own, Comm* c, const Tuning& t)
{
    domain = dom;
    comm = c;
    tune = t;
    dev.fused_rows = (int)t.fused_rows;
    dev.full_rows = (int)t.full_rows;
    dev.lean_tiles = t.no_lean_tiles ? 0 : 1;
    dev.ordered_serial = t.ordered_serial ? 1 : 0;
    const int myrank = c ? c->rank : 0;
    for (int d = 0; d < 3; ++d) {
        periodic[d] = per[d];
        dx[d] = dx_[d];
        bc_type[d][0] = bct[d][0];
        bc_type[d][1] = bct[d][1];
    }
    boxes = bx;
    owner = own;
    if (owner.empty()) owner.assign(boxes.size(), 0);
    SOMAR_CHECK(owner.size() == boxes.size(), "owner/box count mismatch");

    // ---- patches -------------------------------------------------------------------
    local.clear();
    hpatches.clear();
    long long cursor = 0;
    valid_cells_global = 0;
    for (size_t b = 0; b < boxes.size(); ++b) {
        SOMAR_CHECK(!boxes[b].empty(), "empty box in layout");
        valid_cells_global += boxes[b].numPts();
        if (owner[b] != myrank) continue;
        PatchDesc p;
        std::memset(&p, 0, sizeof(p));
        for (int d = 0; d < 3; ++d) { p.lo[d] = boxes[b].lo[d]; p.n[d] = boxes[b].size(d); }
        p.pj = ((p.n[0] + 2 * FRAME + 1) / 2) * 2;
        p.pk = (long long)p.pj * (p.n[1] + 2 * FRAME);
        const long long elems = p.pk * (p.n[2] + 2 * FRAME);
        p.off = cursor + FRAME * p.pk + (long long)FRAME * p.pj + FRAME;
        cursor += ((elems + 31) / 32) * 32;  // 256-byte aligned patch starts
        hpatches.push_back(p);
        local.push_back((int)b);
    }
    field_elems = cursor;
    dev.staged_coef = !t.no_staged_coef && valid_cells_global >= t.staged_min_cells ? 1 : 0;

    // ---- tiles, XCD-contiguous (march_plan::xcd_order) ------------------------------------------------
    // Tile shape per level: big bricks (8 rows x 32 planes) keep the j/k halo re-reads of a
    // stencil sweep at (8+2)/8 * (32+2)/32 of the ideal; shrink k then j until the level still
    // yields >= 1024 workgroups (4 per CU) so coarse levels keep the chip busy.
    int tj = TILE_J_MAX, tk = TILE_K_MAX;
    auto count_tiles = [&](int tj_, int tk_) {
        long long c = 0;
        for (const PatchDesc& p : hpatches)
            c += (long long)((p.n[0] + TILE_I - 1) / TILE_I) * ((p.n[1] + tj_ - 1) / tj_) * ((p.n[2] + tk_ - 1) / tk_);
        return c;
    };
    while (count_tiles(tj, tk) < 1024 && tk > 1) tk /= 2;
    while (count_tiles(tj, tk) < 1024 && tj > 1) tj /= 2;
    dev.tile_j = tj;
    std::vector<Tile> nat;
    for (int pi = 0; pi < (int)hpatches.size(); ++pi) {
        const PatchDesc& p = hpatches[pi];
        for (int k0 = 0; k0 < p.n[2]; k0 += tk)
            for (int j0 = 0; j0 < p.n[1]; j0 += tj)
                for (int i0 = 0; i0 < p.n[0]; i0 += TILE_I)
                    nat.push_back(march_plan::make_tile(pi, i0, j0, k0, std::min(tk, p.n[2] - k0), 0, 0));
    }
    const int N = (int)nat.size();

    // ---- whole-column tiles for line relaxation (one lane per (i-pair, j) column) ---------------
    {
        std::vector<Tile> ct;
        for (int pi = 0; pi < (int)hpatches.size(); ++pi) {
            const PatchDesc& p = hpatches[pi];
            for (int j0 = 0; j0 < p.n[1]; j0 += ctile_j)
                for (int i0 = 0; i0 < p.n[0]; i0 += TILE_I) ct.push_back(march_plan::make_tile(pi, i0, j0, 0, p.n[2], 0, 0));
        }
        ctiles.assign(std::move(ct), 0);
    }

    // ---- exchange plan ----------------------------------------------------------------
    // Ghost depth 2 (= FRAME): the fused red-black sweep recomputes the red ring of its neighbours
    // and therefore needs phi two deep; every other consumer reads at most one layer.
    int ghost[3];
    for (int d = 0; d < 3; ++d) ghost[d] = active[d] ? FRAME : 0;
    plan = build_exchange_plan(domain, periodic, ghost, boxes, owner, myrank);
    {
        std::vector<int> patch_of(boxes.size(), -1);
        for (int pi = 0; pi < (int)local.size(); ++pi) patch_of[local[pi]] = pi;
        for (CopyItem& it : plan.local) { it.src_patch = patch_of[it.src_patch]; it.dst_patch = patch_of[it.dst_patch]; }
        for (CopyItem& it : plan.send_items) it.src_patch = patch_of[it.src_patch];
        for (CopyItem& it : plan.recv_items) it.dst_patch = patch_of[it.dst_patch];
    }

    // ---- device tables ----------------------------------------------------------------
    d_patches = DevBuf<PatchDesc>::from(hpatches);
    tiles.assign(march_plan::xcd_order(nat), 0);
    d_local_items = DevBuf<CopyItem>::from(plan.local);
    d_send_items = DevBuf<CopyItem>::from(plan.send_items);
    d_recv_items = DevBuf<CopyItem>::from(plan.recv_items);
    d_send_off = DevBuf<long long>::from(plan.send_itemoff);
    d_recv_off = DevBuf<long long>::from(plan.recv_itemoff);
    build_march_tiles(MarchRequest{false, false, march.fused19});
    d_sendbuf = plan.send_total ? DevBuf<double>(plan.send_total) : DevBuf<double>();
    d_recvbuf = plan.recv_total ? DevBuf<double>(plan.recv_total) : DevBuf<double>();

    dev.tiles = tiles.span().p;
    dev.ntiles = N;
    dev.patches = d_patches;
    dev.npatches = (int)hpatches.size();
    // ---- pull exchange: per tile, the local copy items clipped to the tile's one-cell halo (k_gsrb_ortho / k_op_ortho) ----
    {
        const long long pullMax = tune.pull_max_cells;
        long long cells = 0;
        for (const IBox& b : boxes) cells += b.numPts();
        if (plan.peers.empty() && cells <= pullMax && N > 0) {
            std::vector<std::vector<int>> byDst(hpatches.size());
            for (int q = 0; q < (int)plan.local.size(); ++q) byDst[plan.local[q].dst_patch].push_back(q);
            std::vector<CopyItem> titems;
            std::vector<int> tstart(N + 1, 0);
            for (int b = 0; b < N; ++b) {
                const Tile& t = tiles.host()[b];
                const PatchDesc& p = hpatches[t.patch];
                int lo[3] = {t.i0, t.j0, t.k0};
                int hi[3] = {std::min(t.i0 + TILE_I, p.n[0]) - 1, std::min(t.j0 + dev.tile_j, p.n[1]) - 1, t.k0 + t.nk - 1};
                for (int d = 0; d < 3; ++d)
                    if (active[d]) { lo[d] -= 1; hi[d] += 1; }
                tstart[b] = (int)titems.size();
                for (int q : byDst[t.patch]) {
                    const CopyItem& it = plan.local[q];
                    CopyItem c = it;
                    bool empty = false;
                    for (int d = 0; d < 3; ++d) {
                        const int a = std::max(lo[d], it.dst_lo[d]), e = std::min(hi[d], it.dst_lo[d] + it.n[d] - 1);
                        if (e < a) { empty = true; break; }
                        c.dst_lo[d] = a;
                        c.src_lo[d] = it.src_lo[d] + (a - it.dst_lo[d]);
                        c.n[d] = e - a + 1;
                    }
                    if (!empty) titems.push_back(c);
                }
            }
            tstart[N] = (int)titems.size();
            if (titems.empty()) titems.push_back(CopyItem());   // keep the table pointer non-null (one box, no ghosts to move)
            d_tile_items = DevBuf<CopyItem>::from(titems);
            d_tile_item_start = DevBuf<int>::from(tstart);
            dev.tile_items = d_tile_items;
            dev.tile_item_start = d_tile_item_start;
        }
    }
    {
        long long face = 0;
        for (const PatchDesc& q : hpatches) {
            const long long a = (long long)(q.n[0] + 2 * FRAME), b = (long long)(q.n[1] + 2 * FRAME), c = (long long)(q.n[2] + 2 * FRAME);
            face = std::max(face, std::max(a * b, std::max(a * c, b * c)));
        }
        dev.ghost_gy = (int)std::min<long long>(256, std::max<long long>(16, (face + 1023) / 1024));
    }
    // A Dirichlet wall on the HIGH side of direction d: the fused sweep's recomputed red ring needs, in a neighbouring
    // box's frame, the coefficient of that box's top face -- a face no box owns as a low face, so the cell-shaped
    // exchange never carries it (with a Neumann wall the face's flux is dropped and the value is never read).
    for (int d = 0; d < 3; ++d) {
        cf_faces[d].reset();
        if (active[d] && !periodic[d] && bc_type[d][1] == BC_DIRI) {
            int gh[3];
            for (int e = 0; e < 3; ++e) gh[e] = active[e] ? FRAME : 0;
            cf_faces[d].reset(new Copier);
            cf_faces[d]->define_faces(domain, periodic, *this, d, gh, comm);
        }
    }
    refresh_params();
    // the tables above went up with plain hipMemcpy (null stream); the solver's stream is non-blocking and
    // would not wait for them
    SOMAR_HIP(hipDeviceSynchronize());
}

void Level::refresh_params()
{
    StencilParams& P = dev.P;
    for (int d = 0; d < 3; ++d) {
        P.dom_lo[d] = domain.lo[d];
        P.dom_hi[d] = domain.hi[d];
        P.active[d] = active[d];
        P.periodic[d] = periodic[d] ? 1 : 0;
        P.dx[d] = dx[d];
        for (int s = 0; s < 2; ++s) {
            P.neum[d][s] = (!periodic[d] && bc_type[d][s] == BC_NEUM) ? 1 : 0;
            P.diri[d][s] = (!periodic[d] && bc_type[d][s] == BC_DIRI) ? 1 : 0;
        }
    }
    P.alpha = alpha;
    P.beta = beta;
    for (int d = 0; d < 3; ++d) { P.cf_c1[d] = cf_c1[d]; P.cf_c2[d] = cf_c2[d]; }
    dxProduct = active[2] ? dx[0] * dx[1] * dx[2] : dx[0] * dx[1];
}

DevBuf<double> Level::alloc_field() const
{
    DevBuf<double> f = DevBuf<double>::zeros(field_elems > 0 ? field_elems : 1);
    SOMAR_HIP(hipDeviceSynchronize());  // null-stream memset vs the solver's non-blocking stream
    return f;
}

void Level::alloc_metric()
{
    for (int d = 0; d < 3; ++d) {
        if (!jg[d]) jg[d] = alloc_field();
        dev.jg[d] = jg[d];
    }
    if (!jinv) jinv = alloc_field();
    if (!lapdiag) lapdiag = alloc_field();
    dev.jinv = jinv;
    dev.lapdiag = lapdiag;
}

void Level::alloc_cross_metric()
{
    for (int d = 0; d < 3; ++d)
        for (int c = 0; c < 3; ++c) {
            if (c != d && !jgx[d][c]) jgx[d][c] = alloc_field();
            dev.jgf[d][c] = c == d ? dev.jg[d] : jgx[d][c].get();
        }
}

// T = double / float: one code path, the element type decides the pack kernel and the transport's message form
template <class T>
static void exchange_remote_t(const Level& L, T* f, hipStream_t st)
{
    const ExchangePlan& plan = L.plan;
    if (plan.peers.empty()) return;
    T* sb = reinterpret_cast<T*>(L.d_sendbuf.get());
    T* rb = reinterpret_cast<T*>(L.d_recvbuf.get());
    launch_pack(st, L.dev, L.d_send_items, L.d_send_off, (int)plan.send_items.size(), f, sb, true);
    L.comm->neighbor_exchange(sb, rb, plan.peers, plan.soff, plan.scount, plan.roff, plan.rcount, st);
    launch_pack(st, L.dev, L.d_recv_items, L.d_recv_off, (int)plan.recv_items.size(), f, rb, false);
    L.sent_bytes[sizeof(T) == sizeof(float)] += plan.send_total * (long long)sizeof(T);
}

template <class T>
static void exchange_t(const Level& L, T* f, hipStream_t st)
{
    // remote first so the wire time overlaps the local copies
    const ExchangePlan& plan = L.plan;
    const bool remote = !plan.peers.empty();
    T* sb = reinterpret_cast<T*>(L.d_sendbuf.get());
    T* rb = reinterpret_cast<T*>(L.d_recvbuf.get());
    if (remote) {
        launch_pack(st, L.dev, L.d_send_items, L.d_send_off, (int)plan.send_items.size(), f, sb, true);
        L.comm->neighbor_exchange(sb, rb, plan.peers, plan.soff, plan.scount, plan.roff, plan.rcount, st);
    }
    launch_copy_items(st, L.dev, L.d_local_items, (int)plan.local.size(), f);
    if (remote) {
        launch_pack(st, L.dev, L.d_recv_items, L.d_recv_off, (int)plan.recv_items.size(), f, rb, false);
        L.sent_bytes[sizeof(T) == sizeof(float)] += plan.send_total * (long long)sizeof(T);
    }
}

void Level::exchange_remote(double* f, hipStream_t st) const { exchange_remote_t(*this, f, st); }
void Level::exchange_remote(float* f, hipStream_t st) const { exchange_remote_t(*this, f, st); }

void Level::exchange_local(double* f, hipStream_t st) const
{
    launch_copy_items(st, dev, d_local_items, (int)plan.local.size(), f);
}
void Level::exchange_local(float* f, hipStream_t st) const
{
    launch_copy_items(st, dev, d_local_items, (int)plan.local.size(), f);
}

void Level::exchange(double* f, hipStream_t st) const { exchange_t(*this, f, st); }
void Level::exchange(float* f, hipStream_t st) const { exchange_t(*this, f, st); }

static void copy3d(void* dst, size_t dpitchB, size_t dheight, int dx0, int dy0, int dz0, const void* src,
                   size_t spitchB, size_t sheight, int sx0, int sy0, int sz0, const int n[3], hipMemcpyKind kind,
                   hipStream_t st)
{
    hipMemcpy3DParms p;
    std::memset(&p, 0, sizeof(p));
    p.srcPtr = make_hipPitchedPtr(const_cast<void*>(src), spitchB, spitchB / sizeof(double), sheight);
    p.dstPtr = make_hipPitchedPtr(dst, dpitchB, dpitchB / sizeof(double), dheight);
    p.srcPos = make_hipPos((size_t)sx0 * sizeof(double), sy0, sz0);
    p.dstPos = make_hipPos((size_t)dx0 * sizeof(double), dy0, dz0);
    p.extent = make_hipExtent((size_t)n[0] * sizeof(double), n[1], n[2]);
    p.kind = kind;
    SOMAR_HIP(hipMemcpy3DAsync(&p, st));
}

void Level::upload(double* field, int patch, const double* host, const IBox& hostbox, const IBox& region,
                   hipStream_t st) const
{
    if (region.empty()) return;
    const PatchDesc& p = hpatches[patch];
    // device "volume": origin at the frame corner of the patch
    double* base = field + (p.off - FRAME * p.pk - (long long)FRAME * p.pj - FRAME);
    int n[3] = {region.size(0), region.size(1), region.size(2)};
    for (int d = 0; d < 3; ++d)
        SOMAR_CHECK(region.lo[d] - p.lo[d] >= -FRAME && region.hi[d] - p.lo[d] < p.n[d] + FRAME &&
                        region.lo[d] >= hostbox.lo[d] && region.hi[d] <= hostbox.hi[d],
                    "upload region outside patch frame or host box");
    copy3d(base, (size_t)p.pj * 8, (size_t)(p.pk / p.pj), region.lo[0] - p.lo[0] + FRAME,
           region.lo[1] - p.lo[1] + FRAME, region.lo[2] - p.lo[2] + FRAME, host, (size_t)hostbox.size(0) * 8,
           (size_t)hostbox.size(1), region.lo[0] - hostbox.lo[0], region.lo[1] - hostbox.lo[1],
           region.lo[2] - hostbox.lo[2], n, hipMemcpyHostToDevice, st);
}

void Level::download(const double* field, int patch, double* host, const IBox& hostbox, const IBox& region,
                     hipStream_t st) const
{
    if (region.empty()) return;
    const PatchDesc& p = hpatches[patch];
    const double* base = field + (p.off - FRAME * p.pk - (long long)FRAME * p.pj - FRAME);
    int n[3] = {region.size(0), region.size(1), region.size(2)};
    for (int d = 0; d < 3; ++d)
        SOMAR_CHECK(region.lo[d] - p.lo[d] >= -FRAME && region.hi[d] - p.lo[d] < p.n[d] + FRAME &&
                        region.lo[d] >= hostbox.lo[d] && region.hi[d] <= hostbox.hi[d],
                    "download region outside patch frame or host box");
    copy3d(host, (size_t)hostbox.size(0) * 8, (size_t)hostbox.size(1), region.lo[0] - hostbox.lo[0],
           region.lo[1] - hostbox.lo[1], region.lo[2] - hostbox.lo[2], base, (size_t)p.pj * 8,
           (size_t)(p.pk / p.pj), region.lo[0] - p.lo[0] + FRAME, region.lo[1] - p.lo[1] + FRAME,
           region.lo[2] - p.lo[2] + FRAME, n, hipMemcpyDeviceToHost, st);
}

// ---- caller arrays by shape: host memory (copy3d), device memory (box_io.hip) ----------------------------------------
BoxIoBoxes Level::io_boxes(int patch, const BoxIoShape& s) const
{
    const IBox& valid = boxes[local[patch]];
    BoxIoBoxes b;
    if (s.face >= 0) {
        b.caller = valid;
        b.caller.hi[s.face] += 1;
        b.region = b.caller;
    } else {
        b.caller = valid.grow(s.ghost);
        b.region = valid.grow(s.grow);
    }
    return b;
}

void check_shape(const BoxIoShape& s)
{
    SOMAR_CHECK(s.face >= -1 && s.face < 3 && s.ncomp >= 1 && s.ncomp <= 3, "box I/O: bad face direction / component count");
    for (int d = 0; d < 3; ++d) {
        SOMAR_CHECK(s.grow[d] >= 0 && s.grow[d] <= s.ghost[d], "box I/O: region outside the caller's box");
        SOMAR_CHECK(s.grow[d] <= FRAME, "ghost wider than device frame");
        SOMAR_CHECK(s.face < 0 || s.ghost[d] == 0, "box I/O: face arrays carry no ghosts");
    }
}

void Level::move_host(double* const field[3], int patch, double* host, const BoxIoShape& s, bool to_level, hipStream_t st) const
{
    check_shape(s);
    SOMAR_CHECK(patch >= 0 && patch < npatches(), "bad patch index: patch out of range");
    SOMAR_CHECK(host != nullptr, "null pointer");
    const BoxIoBoxes b = io_boxes(patch, s);
    for (int c = 0; c < s.ncomp; ++c) {
        SOMAR_CHECK(field[c] != nullptr, "box I/O: no such level array");
        double* h = host + (long long)c * b.caller.numPts();
        if (to_level) upload(field[c], patch, h, b.caller, b.region, st);
        else download(field[c], patch, h, b.caller, b.region, st);
    }
}

void Level::check_dev_ptrs(const double* const* dev, const BoxIoShape& s, const char* what) const
{
    check_shape(s);
    SOMAR_CHECK(dev != nullptr, std::string(what) + ": null pointer table");
    if (npatches() == 0) return;
    hipPointerAttribute_t mine;
    SOMAR_HIP(hipPointerGetAttributes(&mine, d_patches.get()));
    for (int p = 0; p < npatches(); ++p) {
        if (!dev[p]) continue;
        hipPointerAttribute_t a;
        const hipError_t e = hipPointerGetAttributes(&a, dev[p]);
        if (e != hipSuccess) (void)hipGetLastError();   // an unknown pointer leaves a sticky error behind
        if (e != hipSuccess || a.type != hipMemoryTypeDevice || a.isManaged || a.device != mine.device)
            throw Error(-1, std::string(what) + "[" + std::to_string(p) + "] (local patch " + std::to_string(p) + ", box " +
                                std::to_string(local[p]) + ") is not a device pointer on this solver's device " +
                                std::to_string(mine.device));
        // where the runtime knows the allocation the pointer lies in, the whole array must fit into it
        void* base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<double*>(dev[p])) != hipSuccess) { (void)hipGetLastError(); continue; }
        const size_t need = (size_t)io_boxes(p, s).caller.numPts() * s.ncomp * sizeof(double);
        const size_t at = (size_t)(reinterpret_cast<const char*>(dev[p]) - static_cast<const char*>(base));
        if (at > size || need > size - at)
            throw Error(-1, std::string(what) + "[" + std::to_string(p) + "]: the allocation ends before the array of local patch " +
                                std::to_string(p) + " does (" + std::to_string(need) + " bytes needed, " + std::to_string(size - at) + " there)");
    }
}

Level::BoxIoTable& Level::io_table(const BoxIoShape& s)
{
    for (auto& t : io_tables_)
        if (t->shape == s) return *t;
    check_shape(s);
    std::vector<BoxIoItem> items;
    long long ntiles = 0;
    for (int p = 0; p < npatches(); ++p) {
        const PatchDesc& pd = hpatches[p];
        const BoxIoBoxes b = io_boxes(p, s);
        const IBox &cb = b.caller, &region = b.region;
        if (region.empty()) continue;
        for (int d = 0; d < 3; ++d)
            SOMAR_CHECK(region.lo[d] - pd.lo[d] >= -FRAME && region.hi[d] - pd.lo[d] < pd.n[d] + FRAME &&
                            region.lo[d] >= cb.lo[d] && region.hi[d] <= cb.hi[d],
                        "box I/O region outside patch frame or caller box");
        for (int c = 0; c < s.ncomp; ++c) {
            BoxIoItem it;
            std::memset(&it, 0, sizeof(it));
            for (int d = 0; d < 3; ++d) { it.clo[d] = cb.lo[d]; it.rlo[d] = region.lo[d]; it.n[d] = region.size(d); }
            it.cpj = cb.size(0);
            it.cpk = (long long)cb.size(0) * cb.size(1);
            it.coff = (long long)c * cb.numPts();
            it.patch = p;
            it.comp = c;
            it.slot = p;
            const long long nij = (long long)it.n[0] * it.n[1];
            SOMAR_CHECK(nij < (1LL << 31), "box I/O: an i-j plane of 2^31 cells or more");
            it.tiles_ij = (int)((nij + BIO_THREADS - 1) / BIO_THREADS);
            SOMAR_CHECK(ntiles < (1LL << 31), "box I/O: too many tiles");
            it.tile0 = (int)ntiles;
            ntiles += (long long)it.tiles_ij * ((it.n[2] + BIO_KC - 1) / BIO_KC);
            items.push_back(it);
        }
    }
    SOMAR_CHECK(ntiles < (1LL << 31), "box I/O: too many tiles");
    std::unique_ptr<BoxIoTable> t(new BoxIoTable);
    t->shape = s;
    t->nitems = (int)items.size();
    t->ntiles = (int)ntiles;
    t->d_items = DevBuf<BoxIoItem>::from(items);
    t->hptrs.assign(std::max(npatches(), 1), nullptr);
    t->d_ptrs = DevBuf<double*>(t->hptrs.size());
    io_tables_.push_back(std::move(t));
    return *io_tables_.back();
}

void Level::run_box_io(double* const field[3], double* const* dev, const BoxIoShape& s, hipStream_t st, bool to_level, bool checked)
{
    if (!checked) check_dev_ptrs(dev, s, to_level ? "upload_dev" : "download_dev");
    for (int c = 0; c < s.ncomp; ++c) SOMAR_CHECK(field[c] != nullptr, "box I/O: no such level array");
    BoxIoTable& t = io_table(s);
    if (t.nitems == 0) return;
    for (int p = 0; p < npatches(); ++p) t.hptrs[p] = dev[p];
    SOMAR_HIP(hipMemcpyAsync(t.d_ptrs, t.hptrs.data(), t.hptrs.size() * sizeof(double*), hipMemcpyHostToDevice, st));
    launch_box_io(st, this->dev, t.d_items, t.d_ptrs, t.nitems, t.ntiles, field, to_level);
    SOMAR_HIP(hipStreamSynchronize(st));   // the calls block; t.hptrs and the caller's table are free again
}

void Level::upload_dev(double* const field[3], const double* const* dev, const BoxIoShape& s, hipStream_t st, bool checked)
{
    run_box_io(field, const_cast<double* const*>(dev), s, st, true, checked);   // the kernel only reads them in this direction
}

void Level::download_dev(double* const field[3], double* const* dev, const BoxIoShape& s, hipStream_t st, bool checked)
{
    run_box_io(field, dev, s, st, false, checked);
}

}  // namespace somar
