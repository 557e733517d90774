// Stand-alone host program for the host side of the fused patch path: patch_shape, build_patch_work and build_chain_items
// (csrc/vrt_patch.cpp, compiled along) and ChainLaunch::select (csrc/vrt_internal.h).  Built by tests/test_patch_host.py
// with g++ -fsanitize=address,undefined and run as a child process.  The HIP calls behind DevBuf are faked below (device
// memory is malloc, hipMalloc can be told to fail at its k-th call).  The patch index is made by hand and has no geometric
// meaning: three angles (two up, one down), four layers, 0, 1, 9 or 17 patches per (angle, layer).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "vrt_internal.h"

namespace {
std::map<void *, size_t> live_dev;      // address -> bytes
long bad_release = 0, mallocs = 0, fail_at = -1;
std::string last_error;
int checks = 0;
}  // namespace

// ---- the fake runtime ------------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes)
{
    if (mallocs++ == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    live_dev[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    if (!live_dev.erase(p)) { bad_release++; return hipErrorInvalidValue; }
    std::free(p);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipHostFree(void *) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "error"; }
void vrt_plan_destroy(vrt_plan *) {}
void vrt_grid_destroy(vrt_grid *) {}
}

namespace vrt {
void set_error(const std::string &msg) { last_error = msg; }
int fail(int code, const std::string &msg)
{
    last_error = msg;
    return code;
}
void raster_locator_delete(RasterLocator *) {}
bool patch_shape_exists(int K, int Q, int NT)      // the instantiated shapes (vrt_patch.hip: VRT_PATCH_SHAPES)
{
    static const int shapes[9][3] = {{1, 1, 256}, {1, 1, 512}, {1, 1, 1024}, {2, 1, 256}, {2, 1, 512}, {1, 2, 256}, {1, 2, 512}, {1, 2, 1024}, {2, 2, 512}};
    for (const auto &s : shapes)
        if (K == s[0] && Q == s[1] && NT == s[2]) return true;
    return false;
}
}  // namespace vrt

using namespace vrt;

namespace {

#define CHECK(cond)                                                                  \
    do {                                                                             \
        checks++;                                                                    \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

constexpr int kA = 3, kMaxL = 4;
constexpr int64_t kN = 2271;
constexpr int kPadCode = 0x40000000, kReduceCode = (int)0x80000000u;

// the hand-made index
struct Index {
    std::vector<int32_t> first;
    std::vector<int4> rec;
    std::vector<int2> rec2;
    std::vector<int64_t> dep_off;
    std::vector<int32_t> deps;
    std::vector<int> dir_of_active{+1, +1, -1};
    std::vector<int64_t> reduced[2] = {{1, 41, 1141, 1741, 2271}, {1, 51, 751, 2051, 2271}};
    std::vector<int> layer_of_patch;
    int dir(int a) const { return dir_of_active[(size_t)a] > 0 ? 0 : 1; }
    PatchIndex view() const
    {
        return PatchIndex{first, rec, rec2, dep_off, deps, dir_of_active, {&reduced[0], &reduced[1]}, kMaxL, kN};
    }
    int32_t first_of(int a, int layer) const { return first[(size_t)a * (kMaxL + 2) + (size_t)layer]; }
};

Index make_index()
{
    // patches per (angle, layer 1 .. 4): runs of the eight that are empty, single and uneven
    static const int count[kA][kMaxL + 1] = {{0, 0, 17, 9, 1}, {0, 0, 1, 0, 17}, {0, 0, 9, 17, 0}};
    Index ix;
    ix.first.assign((size_t)kA * (kMaxL + 2), 0);
    ix.dep_off.push_back(0);
    int32_t entry = 0;
    for (int a = 0; a < kA; a++) {
        const std::vector<int64_t> &r = ix.reduced[ix.dir(a)];
        for (int layer = 0; layer <= kMaxL + 1; layer++) {
            ix.first[(size_t)a * (kMaxL + 2) + (size_t)layer] = (int32_t)ix.rec.size();
            if (layer < 1 || layer > kMaxL) continue;
            int32_t pos = (int32_t)(r[(size_t)layer - 1] - 1);
            const int32_t prev0 = layer >= 2 ? ix.first_of(a, layer - 1) : 0, prevn = layer >= 2 ? ix.first_of(a, layer) - prev0 : 0;
            for (int k = 0; k < count[a][layer]; k++) {
                const int32_t own = 10 + (k * 7 + a) % 20;                  // (17 x 29 sites fit the smallest layer)
                ix.rec.push_back(make_int4(entry, own + 3, pos, own));
                ix.rec2.push_back(make_int2(1 + k % 5, a));
                ix.layer_of_patch.push_back(layer);
                for (int t = 0; t < std::min(prevn, 1 + k % 3); t++) ix.deps.push_back(prev0 + (k + t) % prevn);
                ix.dep_off.push_back((int64_t)ix.deps.size());
                entry += own + 3;
                pos += own;
            }
            CHECK(pos <= r[(size_t)layer] - 1);
        }
    }
    return ix;
}

// the run of the eight that item t of m falls into, and its place there
void run_of(size_t m, size_t t, int &x, size_t &place)
{
    x = 0;
    while (!(t < m * (size_t)(x + 1) / 8)) x++;
    place = t - m * (size_t)x / 8;
}

// a layer's patches of `angles` in the launches' order: (first owned position, place in angles)
std::vector<int32_t> ordered(const Index &ix, const std::vector<int> &angles, int layer)
{
    std::vector<std::pair<std::pair<int, int>, int32_t>> v;
    for (size_t j = 0; j < angles.size(); j++)
        for (int32_t q = ix.first_of(angles[j], layer); q < ix.first_of(angles[j], layer + 1); q++)
            v.push_back({{ix.rec[(size_t)q].z, (int)j}, q});
    std::sort(v.begin(), v.end());
    std::vector<int32_t> out;
    for (const auto &e : v) out.push_back(e.second);
    return out;
}

bool is_zero(const int4 &v) { return v.x == 0 && v.y == 0 && v.z == 0 && v.w == 0; }
bool same(const int4 &a, const int4 &b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

void check_chain(const Index &ix, int nblock, int nsplit, bool with_reduce)
{
    struct { std::vector<int4> items; std::vector<int32_t> deps; ChainItems set; int *q_off; bool segments_even; } b;
    CHECK(build_chain_items(ix.view(), nblock, nsplit, with_reduce, b.items, b.deps, b.set) == VRT_OK);
    b.q_off = b.set.q_off;
    b.segments_even = b.set.segments_even;
    CHECK(b.segments_even);
    CHECK(b.items.size() % 3 == 0 && b.q_off[0] == 0 && b.q_off[8] == (int)(b.items.size() / 3));
    const int len = b.q_off[1] - b.q_off[0];
    for (int x = 0; x < 8; x++) CHECK(b.q_off[x + 1] - b.q_off[x] == len);
    CHECK(b.deps.size() >= ix.deps.size() && std::equal(ix.deps.begin(), ix.deps.end(), b.deps.begin()));
    std::vector<int> dir_angles[2];
    for (int a = 0; a < kA; a++) dir_angles[ix.dir(a)].push_back(a);
    // where every patch has to be: queue = its run of the (layer, direction) order
    std::vector<int> queue_of(ix.rec.size(), -1);
    for (int layer = 2; layer <= kMaxL; layer++)
        for (int d = 0; d < 2; d++) {
            const std::vector<int32_t> o = ordered(ix, dir_angles[d], layer);
            for (size_t t = 0; t < o.size(); t++) {
                size_t place;
                run_of(o.size(), t, queue_of[(size_t)o[t]], place);
            }
        }
    auto item = [&](int x, int i, int k) -> const int4 & { return b.items[3 * (size_t)(b.q_off[x] + i) + (size_t)k]; };
    // the segment of an item: solve items of (layer, direction) 3 layer + d; J_dir items of layer l follow the solve items
    // of layer l + 1: 3 (l + 1) + 2; -1: padding
    auto segment = [&](int x, int i) {
        const int4 &i0 = item(x, i, 0);
        if (i0.z == kPadCode) return -1;
        const int d = (i0.w >> 6) & 1;
        if (i0.z != kReduceCode) return 3 * (i0.w >> 16) + d;
        const std::vector<int64_t> &r = ix.reduced[d];
        int layer = 1;
        while (layer < kMaxL && !(i0.x < r[(size_t)layer] - 1)) layer++;
        return 3 * (layer + 1) + 2;
    };
    // the queues advance through the segments in step: at every place the items of the eight queues belong to ONE segment,
    // the segments follow each other in order, and a queue's padding stands at the end of its share of a segment
    std::vector<int> seg_at((size_t)len, -1);
    for (int i = 0; i < len; i++) {
        for (int x = 0; x < 8; x++) {
            const int s = segment(x, i);
            if (s < 0) continue;
            CHECK(seg_at[(size_t)i] < 0 || seg_at[(size_t)i] == s);
            seg_at[(size_t)i] = s;
        }
        CHECK(seg_at[(size_t)i] >= 0);                       // (a place where every queue pads would be a wasted round)
        CHECK(i == 0 || seg_at[(size_t)i] >= seg_at[(size_t)i - 1]);
    }
    for (int x = 0; x < 8; x++)
        for (int i = 0; i + 1 < len; i++)
            if (segment(x, i) < 0 && segment(x, i + 1) >= 0) CHECK(seg_at[(size_t)i + 1] > seg_at[(size_t)i]);
    std::vector<int> seen(ix.rec.size() * (size_t)nsplit, 0);
    std::vector<std::pair<int, int>> tiles[2][8];            // [direction][split]: the J_dir items' ranges
    CHECK(nsplit <= 8);
    for (int x = 0; x < 8; x++)
        for (int i = 0; i < len; i++) {
            const int4 &i0 = item(x, i, 0), &i1 = item(x, i, 1), &i2 = item(x, i, 2);
            if (i0.z == kPadCode) {                          // the padding code and nothing else
                CHECK(i0.x == 0 && i0.y == 0 && i0.w == 0 && is_zero(i1) && is_zero(i2));
                continue;
            }
            const int d = (i0.w >> 6) & 1, s = (i0.w >> 7) & 511;
            CHECK(s < nsplit);
            CHECK(i1.x >= 0 && i1.y >= 0 && (size_t)i1.x + (size_t)i1.y <= b.deps.size());
            if (i0.z == kReduceCode) {
                CHECK(with_reduce && is_zero(i2) && i1.z == 0 && (i0.w >> 16) == 0 && (i0.w & 63) == 0);
                CHECK(i1.w == nblock / nsplit + (s < nblock % nsplit ? 1 : 0));
                if (s == 0) {                                // the splits of a range next to each other; their steps sum to nblock
                    int steps = 0;
                    for (int t = 0; t < nsplit; t++) {
                        CHECK(i + t < len);
                        const int4 &j0 = item(x, i + t, 0), &j1 = item(x, i + t, 1);
                        CHECK(j0.x == i0.x && j0.y == i0.y && j0.z == kReduceCode && j0.w == ((d << 6) | (t << 7)));
                        CHECK(j1.x == i1.x && j1.y == i1.y);
                        steps += j1.w;
                    }
                    CHECK(steps == nblock);
                }
                tiles[d][s].push_back({i0.x, i0.y});
                // its dependencies: exactly the patches of its layer and direction that overlap [lo, hi)
                const int layer = (segment(x, i) - 2) / 3 - 1;
                std::set<int32_t> want, have(b.deps.begin() + i1.x, b.deps.begin() + i1.x + i1.y);
                if (layer >= 2)
                    for (int a : dir_angles[d])
                        for (int32_t q = ix.first_of(a, layer); q < ix.first_of(a, layer + 1); q++)
                            if (ix.rec[(size_t)q].z < i0.y && ix.rec[(size_t)q].z + ix.rec[(size_t)q].w > i0.x) want.insert(q);
                CHECK(have == want && (int)have.size() == i1.y);
                CHECK((size_t)i1.x >= ix.deps.size());
                continue;
            }
            const int32_t pq = i1.z;
            CHECK(pq >= 0 && (size_t)pq < ix.rec.size());
            const int4 &rec = ix.rec[(size_t)pq];
            const int2 &rec2 = ix.rec2[(size_t)pq];
            const int layer = ix.layer_of_patch[(size_t)pq];
            CHECK(i0.x == rec.x && i0.y == rec.z && i0.z == (rec.y | (rec.w << 10) | (rec2.x << 20)));
            CHECK(i0.w == (rec2.y | (ix.dir(rec2.y) << 6) | (s << 7) | (layer << 16)));
            CHECK(i1.x == ix.dep_off[(size_t)pq] && i1.y == ix.dep_off[(size_t)pq + 1] - ix.dep_off[(size_t)pq] && i1.w == 0);
            const std::vector<int64_t> &r = ix.reduced[d];
            CHECK(i2.x == r[(size_t)layer - 1] - 1 && i2.y == r[(size_t)layer] - 1 && i2.z == 0 && i2.w == 0);
            CHECK(x == queue_of[(size_t)pq]);
            CHECK(s == 0 || item(x, i - 1, 1).z == pq);      // the splits of a patch next to each other, in order
            seen[(size_t)pq * (size_t)nsplit + (size_t)s]++;
        }
    for (size_t q = 0; q < ix.rec.size(); q++)
        for (int s = 0; s < nsplit; s++) CHECK(seen[q * (size_t)nsplit + (size_t)s] == (ix.layer_of_patch[q] >= 2 ? 1 : 0));
    for (int d = 0; d < 2; d++)
        for (int s = 0; s < nsplit; s++) {
            std::vector<std::pair<int, int>> &t = tiles[d][s];
            if (!with_reduce) { CHECK(t.empty()); continue; }
            std::sort(t.begin(), t.end());
            int at = 0;
            for (const auto &r : t) { CHECK(r.first == at && r.second > r.first); at = r.second; }
            CHECK(at == kN);
        }
}

void check_work(const Index &ix, const std::vector<int32_t> &group_angles, const std::vector<int> &group_off)
{
    const int G = (int)group_off.size() - 1;
    struct { std::vector<int4> work; std::vector<int64_t> off; int64_t padding = -1; } w;
    build_patch_work(ix.view(), G, group_angles, group_off, w.work, w.off, w.padding);
    CHECK(w.off.size() == (size_t)G * (kMaxL + 2) + 1 && w.off.back() == (int64_t)(w.work.size() / 2));
    std::vector<int> seen(ix.rec.size(), 0);
    int64_t slots_all = 0, patches_all = 0;
    for (int gi = 0; gi < G; gi++) {
        const std::vector<int> angles(group_angles.begin() + group_off[(size_t)gi], group_angles.begin() + group_off[(size_t)gi + 1]);
        for (int layer = 0; layer <= kMaxL + 1; layer++) {
            const int64_t w0 = w.off[(size_t)gi * (kMaxL + 2) + (size_t)layer], w1 = w.off[(size_t)gi * (kMaxL + 2) + (size_t)layer + 1];
            CHECK(w1 >= w0 && (w1 - w0) % 8 == 0);
            if (layer < 2 || layer > kMaxL) { CHECK(w1 == w0); continue; }
            const std::vector<int32_t> o = ordered(ix, angles, layer);
            CHECK(w1 - w0 == (int64_t)(o.size() + 7) / 8 * 8);
            std::vector<char> filled((size_t)(w1 - w0), 0);
            for (size_t t = 0; t < o.size(); t++) {          // slot place * 8 + x holds item `place` of run x
                int x;
                size_t place;
                run_of(o.size(), t, x, place);
                const size_t slot = (size_t)w0 + place * 8 + (size_t)x;
                const int32_t q = o[t];
                const int d = ix.dir(ix.rec2[(size_t)q].y);
                const std::vector<int64_t> &r = ix.reduced[d];
                CHECK(same(w.work[2 * slot], ix.rec[(size_t)q]));
                CHECK(same(w.work[2 * slot + 1], make_int4(ix.rec2[(size_t)q].x, ix.rec2[(size_t)q].y | (d << 16), (int)(r[(size_t)layer - 1] - 1),
                                                           (int)(r[(size_t)layer] - 1))));
                filled[slot - (size_t)w0] = 1;
                seen[(size_t)q]++;
            }
            for (int64_t s = w0; s < w1; s++)
                if (!filled[(size_t)(s - w0)]) CHECK(is_zero(w.work[2 * (size_t)s]) && is_zero(w.work[2 * (size_t)s + 1]));
            slots_all += w1 - w0;
            patches_all += (int64_t)o.size();
        }
    }
    for (size_t q = 0; q < ix.rec.size(); q++) CHECK(seen[q] == (ix.layer_of_patch[q] >= 2 ? 1 : 0));
    CHECK(slots_all == w.off.back() && w.padding == slots_all - patches_all);
}

void check_shapes()
{
    vrt_plan plan;
    plan.patch_ok = true;
    plan.tile_max_layers = 100;
    plan.A = kA;
    int chained = 0, dataflagged = 0, quads = 0, leans = 0;
    for (int f32 = 0; f32 < 2; f32++)
    for (int lg = 0; lg <= 2; lg++)
    for (int K = 1; K <= 2; K++)
    for (int NT : {256, 512})
    for (int quad = 0; quad < 2; quad++)
    for (int lean = 0; lean < 2; lean++)
    for (int chain = 0; chain <= 2; chain++)
    for (int df = 0; df <= 2; df++)
    for (int npair = 1; npair <= 4; npair++)
    for (int Q = 1; Q <= 2; Q++) {
        plan.lg_pair_block = lg; plan.patch_K = K; plan.patch_NT = NT;
        plan.tune.patch_quad = quad; plan.tune.patch_lean = lean; plan.tune.patch_chain = chain; plan.tune.chain_dataflag = df;
        plan.n_patches = 100 * 300;
        const PatchShape s = patch_shape(&plan, npair, f32 != 0, Q);
        CHECK(s.lgB == native_lg(&plan, f32 != 0));
        CHECK(s.quad == 0 || s.quad == 1);
        if (s.quad) CHECK(f32 && K == 1 && npair % 2 == 0 && s.lgB >= 1 && s.Q == 1 && quad);
        CHECK(s.lgS == s.lgB - s.quad);
        CHECK(s.Q == 1 || (s.Q == Q && patch_shape_exists(K, Q, NT)));
        if (s.lean) CHECK(K == 1 && s.Q == 1 && !s.quad && npair >= 2 && lean);
        if (s.chain) CHECK(s.lgS == 0 && K == 1 && NT == 512 && chain != 0);
        if (s.chain_dataflag) CHECK(s.chain && !f32 && s.lgB == 0 && df != 0);
        if (chain == 0) CHECK(!s.chain);
        chained += s.chain; dataflagged += s.chain_dataflag; quads += s.quad; leans += s.lean;
    }
    CHECK(chained > 0 && dataflagged > 0 && quads > 0 && leans > 0);
    // auto: chained up to 1400 (patches of a layer) x (pair blocks), doubles only
    plan.lg_pair_block = 0; plan.patch_K = 1; plan.patch_NT = 512;
    plan.tune = Tuning();
    plan.n_patches = 100 * 350;
    CHECK(patch_shape(&plan, 4, false, 1).chain && !patch_shape(&plan, 5, false, 1).chain);
    CHECK(!patch_shape(&plan, 4, true, 1).chain);
    CHECK(patch_shape(&plan, 2, false, 1).chain_dataflag && !patch_shape(&plan, 3, false, 1).chain_dataflag);
    plan.patch_ok = false;
    const PatchShape none = patch_shape(&plan, 4, true, 2);
    CHECK(none.lgB == 0 && !none.chain && !none.chain_dataflag);
}

void check_cache()
{
    long builds = 0;
    auto make = [&](ChainItems &cs) -> int {
        builds++;
        int rc;
        if ((rc = cs.items.alloc(3)) || (rc = cs.deps.alloc(5))) return rc;
        cs.q_off[8] = 1;
        return VRT_OK;
    };
    {
        ChainLaunch cl;
        std::map<int, std::pair<void *, void *>> addr;
        for (int k = 1; k <= 5; k++) {                       // five keys in turn: four sets alive, the oldest went
            CHECK(cl.select(k, 0, 2, true, make) == VRT_OK);
            CHECK(cl.sets.front().npair == k && cl.sets.size() <= ChainLaunch::kSets && live_dev.size() == 2 * cl.sets.size());
            addr[k] = {cl.sets.front().items.p, cl.sets.front().deps.p};
        }
        CHECK(builds == 5 && cl.sets.size() == 4 && cl.sets.back().npair == 2);
        // a key that returns: no rebuild, the same buffers, now in front; the others keep their order
        CHECK(cl.select(3, 0, 2, true, make) == VRT_OK && builds == 5 && mallocs == 10);
        CHECK(cl.sets.front().npair == 3 && cl.sets.front().items.p == addr[3].first && cl.sets.front().deps.p == addr[3].second);
        CHECK(cl.sets[1].npair == 5 && cl.sets[2].npair == 4 && cl.sets[3].npair == 2);
        // every part of the key counts
        CHECK(cl.select(3, 0, 2, false, make) == VRT_OK && builds == 6 && cl.sets[3].npair == 4);
        CHECK(cl.select(3, 1, 2, true, make) == VRT_OK && builds == 7);
        CHECK(cl.select(3, 0, 3, true, make) == VRT_OK && builds == 8);
        // the least recently used one went each time: key 1 is rebuilt, key 3 (with reduce) is still there
        CHECK(cl.select(3, 0, 2, true, make) == VRT_OK && builds == 8 && cl.sets.front().items.p == addr[3].first);
        CHECK(cl.select(1, 0, 2, true, make) == VRT_OK && builds == 9);
        // an allocation that fails at each position in turn: the owner stays usable, nothing leaks
        for (int pos = 0; pos < 2; pos++) {
            const int front = cl.sets.front().npair;
            fail_at = mallocs + pos;
            CHECK(cl.select(7 + pos, 0, 2, true, make) == VRT_ENOMEM);
            fail_at = -1;
            CHECK(!cl.sets.empty() && cl.sets.size() < ChainLaunch::kSets && cl.sets.front().npair == front);
            CHECK(live_dev.size() == 2 * cl.sets.size());
            for (const ChainItems &cs : cl.sets) CHECK(cs.items.p && cs.deps.p && live_dev.count(cs.items.p) && live_dev.count(cs.deps.p));
            const long before = builds;
            CHECK(cl.select(front, 0, 2, true, make) == VRT_OK && builds == before);
            CHECK(cl.select(7 + pos, 0, 2, true, make) == VRT_OK && builds == before + 1 && cl.sets.front().npair == 7 + pos);
        }
    }
    CHECK(live_dev.empty() && bad_release == 0);
}

}  // namespace

int main()
{
    const Index ix = make_index();
    for (int nsplit : {1, 3})
        for (int reduce = 0; reduce < 2; reduce++) check_chain(ix, 7, nsplit, reduce != 0);
    check_chain(ix, 3, 3, true);                             // (one block per split)
    std::printf("ok chain items\n");
    check_work(ix, {0, 1, 2}, {0, 3});
    check_work(ix, {2, 1, 0}, {0, 1, 3});
    check_work(ix, {1, 2, 0}, {0, 1, 1, 3});                 // (a group without angles)
    std::printf("ok work lists\n");
    check_shapes();
    std::printf("ok shapes\n");
    check_cache();
    std::printf("ok cache\n");
    std::printf("%d checks, no allocation outlived its owner\n", checks);
    return 0;
}
