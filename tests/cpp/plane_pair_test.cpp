// plane_pair_test.cpp -- the source/destination rule of the post-process chain (amatsukaze_amd/csrc/plane_pair.hpp), compiled with plain
// g++ (tests/test_plane_pair_host.py), once more with the address and undefined-behaviour sanitizers.
//   1. planes_touch against a byte map: every byte of [first byte of frame 0, last byte of frame n - 1] of each source plane is marked,
//      and a placement of the destination must be refused exactly when one of its planes' ranges holds a marked byte.  One destination
//      plane at a time walks every container offset of an arena that extends a destination frame on either side of the source.
//   2. frames_overlap against the same kind of map, for every stride from 0 to the loosest, and at the two strides around its bound.
//   3. every shared refusal of the four entry points, byte for byte as the entry points worded them before the rule was one file.
//   4. the byte pitch above 2 GiB, which is refused before anything is formed from it.
//   usage: plane_pair_test          (no arguments; prints the number of placements per answer)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "plane_pair.hpp"

using namespace amt;

namespace {
const PlanePairRule kRules[4] = {kRenderPair, kResizePair, kTemporalNRPair, kDebandPair};

// frames of w x h luma containers of es bytes: rows pad containers longer than their samples, frames gap containers behind the last row
struct Geo { int w, h, es, il, pad, gap, n; };
int rowc(const Geo& g, int k) { return k && !g.il ? g.w / 2 : g.w; }
int rowsof(const Geo& g, int k) { return k ? g.h / 2 : g.h; }
int pitchc(const Geo& g, int k) { return rowc(g, k) + g.pad; }
long long frame_bytes(const Geo& g, int k) { return (long long)((rowsof(g, k) - 1) * pitchc(g, k) + rowc(g, k)) * g.es; }
long long stride(const Geo& g, int k) { return (long long)(rowsof(g, k) * pitchc(g, k) + g.gap) * g.es; }
long long extent(const Geo& g, int k) { return (g.n - 1) * stride(g, k) + frame_bytes(g, k); }          // bytes that the n frames of a plane span
int nplanes(const Geo& g) { return g.il ? 2 : 3; }
FrameBatch batch(const Geo& g, const uint8_t* Y, const uint8_t* U, const uint8_t* V)
{
    return FrameBatch{Y, U, V, stride(g, 0), stride(g, 1), pitchc(g, 0), pitchc(g, 1), g.es, g.il, 0};
}
void print(const char* name, const Geo& g)
{
    printf("  %s: %dx%d es %d %s pitch +%d stride +%d frames %d\n", name, g.w, g.h, g.es, g.il ? "interleaved" : "planar", g.pad, g.gap, g.n);
}

int fails = 0;
template <typename F> std::string what_of(F&& f)
{
    try { f(); } catch (const std::runtime_error& e) { return e.what(); }
    return "(accepted)";
}
void expect(const std::string& got, const std::string& want, const char* who, const char* label)
{
    if (got == want) return;
    printf("differs: %s, %s:\n  got  \"%s\"\n  want \"%s\"\n", who, label, got.c_str(), want.c_str());
    ++fails;
}

// ---- 1. the span rule ----
long long answers[2];
bool saw_on_last_byte, saw_behind_last_byte, saw_uv_in_luma;
bool spans_against_the_map()
{
    const PlanePairRule& rule = kTemporalNRPair;
    std::vector<uint8_t> park(4096);                        // where the destination planes that do not walk lie: never in the arena
    for (int es = 1; es <= 2; ++es)
    for (int il = 0; il < 2; ++il)
    for (int sw = 4; sw <= 6; sw += 2)
    for (int spad = 0; spad <= 3; spad += 3)
    for (int sgap = 0; sgap <= 5; sgap += 5)
    for (int nsrc = 1; nsrc <= 3; ++nsrc)
    for (int dw = 4; dw <= 6; dw += 2)
    for (int dpad = 0; dpad <= 3; dpad += 3)
    for (int dgap = 0; dgap <= 5; dgap += 5)
    for (int ndst = 1; ndst <= 2; ++ndst) {
        const Geo s{sw, 4, es, il, spad, sgap, nsrc}, d{dw, 4, es, il, dpad, dgap, ndst};
        const int np = nplanes(s);
        long long around = 0, sext = 0;                     // one destination frame; the source, its planes one behind the other
        for (int p = 0; p < np; ++p) { around += frame_bytes(d, p ? 1 : 0); sext += extent(s, p ? 1 : 0); }
        const long long arena = around + sext + around;
        std::vector<uint8_t> map((size_t)(arena + std::max(extent(d, 0), extent(d, 1))), 0);
        const uint8_t* sp[3] = {map.data() + around, map.data() + around + extent(s, 0), il ? nullptr : map.data() + around + extent(s, 0) + extent(s, 1)};
        for (int p = 0; p < np; ++p) std::memset(const_cast<uint8_t*>(sp[p]), 1, (size_t)extent(s, p ? 1 : 0));
        std::vector<int> marked(map.size() + 1, 0);         // marked[i]: marked bytes below i
        for (size_t i = 0; i < map.size(); ++i) marked[i + 1] = marked[i] + map[i];
        const long long last = around + sext - 1;           // the source's last byte
        if (!map[(size_t)last] || map[(size_t)last + 1]) { printf("the test's own map is wrong\n"); return false; }
        for (int j = 0; j < np; ++j)
            for (long long off = 0; off < arena; off += es) {
                const uint8_t* dp[3] = {park.data(), park.data() + 1024, il ? nullptr : park.data() + 2048};
                dp[j] = map.data() + off;
                const bool want = marked[(size_t)(off + extent(d, j ? 1 : 0))] - marked[(size_t)off] > 0;
                // an interleaved side has no third plane: nothing, a pointer into the other side, a pointer that is no address
                // -- in the batch, which bytes() drops, and planted in what bytes() made, which the plane count keeps out of the spans
                for (int garbage = 0; garbage < (il ? 4 : 1); ++garbage) {
                    const uint8_t* sv = garbage == 0 ? sp[2] : garbage == 2 ? (const uint8_t*)1 : dp[j];
                    const uint8_t* dv = garbage == 0 ? dp[2] : garbage == 2 ? (const uint8_t*)3 : sp[0];
                    PlaneBytes sb = rule.bytes(batch(s, sp[0], sp[1], sv), s.w, s.h), db = rule.bytes(batch(d, dp[0], dp[1], dv), d.w, d.h);
                    bool got = planes_touch(sb, nsrc, db, ndst);
                    if (garbage == 3) {
                        sb.p[2] = sv; db.p[2] = dv;
                        got = planes_touch(sb, nsrc, db, ndst);
                        sb.p[2] = db.p[2] = nullptr;
                    }
                    if (got == want && sb.luma().base2 == 0 && sb.chroma().base2 == lane_addr(il ? nullptr : sp[2]) && db.chroma().base2 == lane_addr(il ? nullptr : dp[2]))
                        continue;
                    printf("differs: destination plane %d at byte %lld of the arena (source at %lld .. %lld), third planes %s: rule %s, map %s\n", j, off,
                           around, last, garbage ? "garbage" : "as they are", got ? "refuses" : "accepts", want ? "refuses" : "accepts");
                    print("source", s); print("destination", d);
                    return false;
                }
                ++answers[want];
                if (es == 1 && off == last && want) saw_on_last_byte = true;
                if (es == 1 && off == last + 1 && !want) saw_behind_last_byte = true;
                if (il && j == 1 && off >= around && off + extent(d, 1) <= around + extent(s, 0) && want) saw_uv_in_luma = true;
            }
    }
    printf("span rule: %lld placements accepted, %lld refused, as the byte map says\n", answers[0], answers[1]);
    if (!answers[0] || !answers[1]) { printf("the domain holds one answer only\n"); return false; }
    if (!saw_on_last_byte || !saw_behind_last_byte || !saw_uv_in_luma) {
        printf("a case that must occur did not: on the last byte %d, behind it %d, UV inside luma %d\n", saw_on_last_byte, saw_behind_last_byte, saw_uv_in_luma);
        return false;
    }
    return true;
}

// ---- 2. the frame-overlap rule ----
bool frames_against_the_map()
{
    const PlanePairRule& rule = kResizePair;
    std::vector<uint8_t> park(4096);
    long long seen[2] = {0, 0};
    for (int es = 1; es <= 2; ++es)
    for (int il = 0; il < 2; ++il)
    for (int w = 4; w <= 6; w += 2)
    for (int pad = 0; pad <= 3; pad += 3)
    for (int k = 0; k < 2; ++k) {                           // the plane kind whose stride walks; the other kind's frames lie far apart
        const Geo g{w, 4, es, il, pad, 5, 2};
        const long long fb = frame_bytes(g, k);
        for (long long st = 0; st <= stride(g, k); st += es) {
            std::vector<uint8_t> map((size_t)(st + fb), 0);
            std::memset(map.data(), 1, (size_t)fb);         // frame 0; frame 1 is [st, st + fb)
            const bool want = std::count(map.begin() + st, map.end(), 1) > 0;
            FrameBatch b = batch(g, park.data(), park.data() + 1024, park.data() + 2048);
            (k ? b.strideUV : b.strideY) = st;
            const PlaneBytes t = rule.bytes(b, g.w, g.h);
            if (frames_overlap(t, 2) != want || frames_overlap(t, 1)) {
                printf("differs: %s stride %lld bytes, frame of %lld bytes: rule %d, map %d; one frame alone %d\n", k ? "chroma" : "luma", st, fb, frames_overlap(t, 2),
                       want, frames_overlap(t, 1));
                print("destination", g);
                return false;
            }
            ++seen[want];
        }
        // the bound itself, through the refusal: a stride of (rows - 1) * pitch + row bytes, and one container less
        for (int ndst = 1; ndst <= 2; ++ndst)
            for (int less = 0; less < 2; ++less) {
                FrameBatch b = batch(g, park.data(), park.data() + 1024, park.data() + 2048);
                (k ? b.strideUV : b.strideY) = fb - less * es;
                const std::vector<uint8_t> src(256);
                const Geo one{4, 4, es, il, 0, 0, 1};
                const PlaneBytes s = rule.bytes(batch(one, src.data(), src.data() + 64, src.data() + 128), 4, 4);
                expect(what_of([&] { rule.disjoint(s, 1, rule.bytes(b, g.w, g.h), ndst); }),
                       ndst == 2 && less ? "[Resize] destination frames overlap each other" : "(accepted)", "[Resize]", "a stride at its bound");
            }
    }
    printf("frame-overlap rule: %lld strides accepted, %lld refused, as the byte map says\n", seen[0], seen[1]);
    return seen[0] && seen[1] && !fails;
}

// ---- 3. the messages ----
AmtGpuSurfaces descriptor(const FrameBatch& b, int bits, int msb_aligned)
{
    return AmtGpuSurfaces{b.Y, b.U, b.V, b.strideY, b.strideUV, b.pitchY, b.pitchUV, bits, b.interleaved, msb_aligned, 0};
}
void messages()
{
    // in the order of kRules: render, resize, temporal NR, deband; null: the entry point has no such refusal
    static const char* const layout[4][2] = {
        {nullptr, nullptr},
        {"[Resize] source: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)",
         "[Resize] destination: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)"},
        {"[TemporalNR] source: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)",
         "[TemporalNR] destination: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)"},
        {"[Deband] source: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)",
         "[Deband] destination: planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)"}};
    static const char* const created[4][2] = {
        {nullptr, nullptr},
        {"[Resize] source: 10 bits, the resizer was created for 8", "[Resize] destination: 10 bits, the resizer was created for 8"},
        {nullptr, nullptr},
        {"[Deband] source: 10 bits, the debander was created for 8", "[Deband] destination: 10 bits, the debander was created for 8"}};
    static const char* const negative[4][2] = {{"[KFMRender] source: negative frame stride", "[KFMRender] destination: negative frame stride"},
                                               {"[Resize] source: negative frame stride", "[Resize] destination: negative frame stride"},
                                               {"[TemporalNR] source: negative frame stride", "[TemporalNR] destination: negative frame stride"},
                                               {"[Deband] source: negative frame stride", "[Deband] destination: negative frame stride"}};
    static const char* const pitch[4][2] = {{"[KFMRender] source: pitch smaller than the row", "[KFMRender] destination: pitch smaller than the row"},
                                            {"[Resize] source: pitch smaller than the row", "[Resize] destination: pitch smaller than the row"},
                                            {"[TemporalNR] source: pitch smaller than the row", "[TemporalNR] destination: pitch smaller than the row"},
                                            {"[Deband] source: pitch smaller than the row", "[Deband] destination: pitch smaller than the row"}};
    static const char* const kind[4] = {
        "[KFMRender] source and destination are not in kind (equal bits, interleaved and MSB shift): the renderer converts no layouts",
        "[Resize] source and destination are not in kind (equal bits, interleaved and MSB shift): the resizer converts no layouts",
        "[TemporalNR] source and destination are not in kind (equal bits, interleaved and MSB shift): the filter converts no layouts", nullptr};
    static const char* const frames[4] = {"[KFMRender] destination frames overlap each other", "[Resize] destination frames overlap each other",
                                          "[TemporalNR] destination frames overlap each other", "[Deband] destination frames overlap each other"};
    static const char* const overlap[4] = {"[KFMRender] the destination's byte range overlaps the source's (no in-place rendering)",
                                           "[Resize] the destination's byte range overlaps the source's (no in-place resize)",
                                           "[TemporalNR] the destination's byte range overlaps the source's (no in-place filtering)",
                                           "[Deband] the destination's byte range overlaps the source's (no in-place filtering: the filter reads neighbours)"};
    static const char* const gib[4] = {"[KFMRender] pitch above 2 GiB", "[Resize] pitch above 2 GiB", "[TemporalNR] pitch above 2 GiB", "[Deband] pitch above 2 GiB"};
    static const char* const which[2] = {"source", "destination"};

    std::vector<uint8_t> mem(4096);
    const uint8_t *Y = mem.data(), *U = Y + 1024, *V = Y + 2048;
    for (int r = 0; r < 4; ++r) {
        const PlanePairRule& rule = kRules[r];
        const char* who = rule.who;
        const bool object = created[r][0] != nullptr;       // resize and deband hold an object of one depth
        const Geo planar{6, 4, 1, 0, 0, 0, 2}, nv12{6, 4, 1, 1, 0, 0, 2}, planar16{6, 4, 2, 0, 0, 0, 2};
        const FrameBatch pl = batch(planar, Y, U, V), il = batch(nv12, Y, U, nullptr), p16 = batch(planar16, Y, U, V);
        const AmtGpuSurfaces pl8 = descriptor(pl, 8, 0), il8 = descriptor(il, 8, 0), msb10 = descriptor(p16, 10, 1), lsb10 = descriptor(p16, 10, 0),
                             msb16 = descriptor(p16, 16, 1);
        for (int side = 0; side < 2; ++side) {
            auto one = [&](const AmtGpuSurfaces& s, FrameBatch b, int width, bool any_layout, int object_bits) {
                return what_of([&] { rule.side(which[side], &s, b, width, any_layout, object_bits); });
            };
            // a good side passes, under either layout rule
            expect(one(pl8, pl, 6, false, 8), "(accepted)", who, "a planar LSB side, planes only");
            expect(one(pl8, pl, 6, true, 8), "(accepted)", who, "a planar LSB side, every layout");
            // planar LSB only against every layout (an MSB-aligned descriptor of 16 bits has no shift and is refused all the same)
            if (layout[r][side]) {
                expect(one(il8, il, 6, false, 8), layout[r][side], who, "interleaved, planes only");
                expect(one(msb10, p16, 6, false, 10), layout[r][side], who, "MSB-aligned, planes only");
                expect(one(msb16, p16, 6, false, 16), layout[r][side], who, "MSB-aligned at 16 bits, planes only");
            }
            expect(one(il8, il, 6, true, 8), "(accepted)", who, "interleaved, every layout");
            expect(one(msb10, p16, 6, true, 10), "(accepted)", who, "MSB-aligned, every layout");
            // the object's bits against none
            expect(one(lsb10, p16, 6, true, 8), object ? created[r][side] : "(accepted)", who, "10 bits where the object, if there is one, has 8");
            // the layout comes before the bits, the bits before the stride, the stride before the pitch
            FrameBatch bad = il;
            bad.strideUV = -bad.strideUV; bad.pitchY = 5;
            if (layout[r][side]) expect(one(descriptor(bad, 10, 0), bad, 6, false, 8), layout[r][side], who, "everything wrong, planes only");
            expect(one(descriptor(bad, 10, 0), bad, 6, true, 8), object ? created[r][side] : negative[r][side], who, "everything wrong, every layout");
            expect(one(descriptor(bad, 8, 0), bad, 6, true, 8), negative[r][side], who, "a negative chroma stride and a short luma pitch");
            FrameBatch neg = pl;
            neg.strideY = -1;
            expect(one(pl8, neg, 6, false, 8), negative[r][side], who, "a negative luma stride");
            // rows: width luma, width / 2 planar chroma, width interleaved chroma
            expect(one(pl8, pl, 8, false, 8), pitch[r][side], who, "luma pitch 6 under width 8");
            FrameBatch narrow = pl;
            narrow.pitchUV = 2;
            expect(one(pl8, narrow, 6, false, 8), pitch[r][side], who, "planar chroma pitch 2 under width 6");
            narrow = il; narrow.pitchUV = 5;
            expect(one(il8, narrow, 6, true, 8), pitch[r][side], who, "interleaved chroma pitch 5 under width 6");
            narrow.pitchUV = 6; narrow.pitchY = 8;
            expect(one(il8, narrow, 6, true, 8), "(accepted)", who, "interleaved chroma pitch 6 at width 6");
        }
        // in kind: equal interleaved, equal shift
        if (kind[r]) {
            FrameBatch shifted = p16;
            shifted.shift = 6;
            expect(what_of([&] { rule.in_kind(il, pl); }), kind[r], who, "NV12 into planes");
            expect(what_of([&] { rule.in_kind(p16, shifted); }), kind[r], who, "planar LSB into planar MSB");
            expect(what_of([&] { rule.in_kind(shifted, shifted); }), "(accepted)", who, "planar MSB into planar MSB");
        }
        // disjoint: the frame-overlap refusal comes first; the cases that must occur, by name
        const Geo far{6, 4, 1, 0, 0, 0, 2};
        std::vector<uint8_t> other(4096);
        const uint8_t* oY = other.data();
        const PlaneBytes s = rule.bytes(pl, 6, 4);
        const uint8_t* last = V + extent(planar, 1) - 1;    // the source's last byte, in its V plane
        auto onto = [&](const uint8_t* y, const uint8_t* u, const uint8_t* v, long long strideY, int ndst) {
            FrameBatch t = batch(far, y, u, v);
            t.strideY = strideY;
            return what_of([&] { rule.disjoint(s, 2, rule.bytes(t, 6, 4), ndst); });
        };
        expect(onto(oY, oY + 1024, oY + 2048, stride(far, 0), 2), "(accepted)", who, "a destination elsewhere");
        expect(onto(Y, oY + 1024, oY + 2048, 23, 2), frames[r], who, "overlapping destination frames on the source");
        expect(onto(Y, oY + 1024, oY + 2048, 23, 1), overlap[r], who, "one destination frame on the source");
        expect(onto(Y, U, V, stride(far, 0), 2), overlap[r], who, "the destination is the source");
        expect(onto(oY, oY + 1024, last, stride(far, 0), 2), overlap[r], who, "a destination plane that starts on the source's last byte");
        expect(onto(oY, oY + 1024, last + 1, stride(far, 0), 2), "(accepted)", who, "a destination plane that starts one byte behind the source's last");
        expect(onto(last + 1 - extent(far, 0), oY + 1024, oY + 2048, stride(far, 0), 2), overlap[r], who, "a destination plane that ends on the source's last byte");
        {
            const PlaneBytes si = rule.bytes(il, 6, 4);
            auto nv12_onto = [&](const uint8_t* y, const uint8_t* uv, const uint8_t* v) {
                return what_of([&] { rule.disjoint(si, 2, rule.bytes(batch(nv12, y, uv, v), 6, 4), 1); });
            };
            expect(nv12_onto(oY, Y + 8, nullptr), overlap[r], who, "an interleaved destination's UV plane inside the source's luma plane");
            expect(nv12_onto(oY, oY + 1024, Y + 8), "(accepted)", who, "an interleaved destination whose unused V points into the source");
        }
        // ---- 4. a byte pitch above 2 GiB is refused before anything is formed from it; 1 << 30 containers of one byte are not
        FrameBatch huge = p16;
        huge.pitchY = (1 << 30) + 16; huge.pitchUV = huge.pitchY / 2;
        expect(what_of([&] { rule.side("source", &lsb10, huge, huge.pitchY, true, 10); }), "(accepted)", who, "rows of 2^30 + 16 containers fit their pitch");
        expect(what_of([&] { rule.bytes(huge, huge.pitchY, 4); }), gib[r], who, "2^30 + 16 containers of 16 bits");
        huge.pitchY = 16; huge.pitchUV = (1 << 30) + 16;
        expect(what_of([&] { rule.bytes(huge, 16, 4); }), gib[r], who, "a chroma pitch of 2^30 + 16 containers of 16 bits");
        huge = pl;
        huge.pitchY = 1 << 30; huge.pitchUV = 1 << 29;
        expect(what_of([&] { const PlaneBytes b = rule.bytes(huge, 1 << 30, 4); if (b.pitch[0] != 1 << 30 || b.row[0] != 1 << 30) throw std::runtime_error("wrong bytes"); }),
               "(accepted)", who, "2^30 containers of 8 bits");
        huge = p16;
        huge.pitchY = (1 << 30) - 1; huge.pitchUV = 1 << 29;
        expect(what_of([&] { if (rule.bytes(huge, (1 << 30) - 2, 4).pitch[0] != INT32_MAX - 1) throw std::runtime_error("wrong bytes"); }), "(accepted)", who,
               "2^30 - 1 containers of 16 bits");
    }
}
} // namespace

int main()
{
    if (!spans_against_the_map() || !frames_against_the_map()) return 1;
    messages();
    if (fails) { printf("%d messages differ\n", fails); return 1; }
    printf("no difference\n");
    return 0;
}
