// host_queries.cpp -- what the size queries and the plan builder of llicti_amd/csrc/host_plan.hpp answer for a fixed list of batches, one line
// per query, and what the admission rules of the whole-batch calls refuse.  Plain g++, beside tests/sanitize_host.cpp:
//   - stdout is compared byte for byte with tests/golden/host_queries.txt (tests/test_host_cpu.py), which was recorded BEFORE the host layer's
//     rules were given single homes: a change of the host layer that moves a workspace size, a container bound, a plan's `uniform` form or a
//     cache key shows up as a differing line;
//   - the bound on a stream's bits (check_stream_bits) is walked to its exact boundary in every lane kind; the heights found are recorded lines too;
//   - every admission function is then called with one faulty input per rule: LLICTI_EINVAL, and the message starts with the caller's prefix.
// tests/sanitize_host.sh runs it under AddressSanitizer + UBSan too.
#include <stdio.h>
#include <stdlib.h>

#include "../llicti_amd/csrc/host_plan.hpp"

#define REQUIRE(c)                                                                      \
    do {                                                                                \
        if (!(c)) { fprintf(stderr, "FAILED %s (%s:%d): last error '%s'\n", #c, __FILE__, __LINE__, g_err.c_str()); exit(1); } \
    } while (0)

// ---- the two calls whose spelling belongs to host_plan.hpp: the resolver of one side's modes, and the plan builder
static bool side_modes(const std::vector<int> &modes, int B, int *ME, std::vector<int> &Ms)
{
    return resolve_modes("host_queries", modes.data(), (int)modes.size(), B, ME, Ms) == 0;
}
static void plan_of(Plan &p, int B, const int *Hs, const int *Ws, int ME, const std::vector<int> &Ms, int nlev, bool ragged)
{
    build_plan(p, PlanSpec{ B, Hs, Ws, ME, modes_ptr(Ms), nlev, ragged });
}
// ----

struct Sizes { const char *name; std::vector<int> Hs, Ws; };
struct Modes { const char *name; std::vector<int> m; };

static const int ac = LLICTI_MODE_AC, r8 = LLICTI_MODE_RANS(8), w14 = LLICTI_MODE_RANS_WIDE(14), x64 = LLICTI_MODE_RANS_X(64), xa3 = LLICTI_MODE_RANS_X_AUTO(3),
                 x4 = LLICTI_MODE_RANS_X(4), x8 = LLICTI_MODE_RANS_X(8), x16 = LLICTI_MODE_RANS_X(16), x18 = LLICTI_MODE_RANS_X(18), x19 = LLICTI_MODE_RANS_X(19),
                 xa10 = LLICTI_MODE_RANS_X_AUTO(10), bad = 0x777;

static void query(const Sizes &s, const Modes &src, const std::vector<Modes> &targets, int nlev)
{
    const int B = (int)s.Hs.size();
    const int *Hs = s.Hs.data(), *Ws = s.Ws.data();
    printf("L%d %s %s: workspace %zu\n", nlev, s.name, src.name, plan_workspace_bytes_vm(B, Hs, Ws, src.m.data(), (int)src.m.size(), nlev));
    int ME = 0;
    std::vector<int> Ms;
    if (check_dims_v(B, Hs, Ws) || !side_modes(src.m, B, &ME, Ms)) printf("L%d %s %s: no plan\n", nlev, s.name, src.name);
    else
        for (int ragged = 0; ragged < 2; ++ragged) {
            Plan p;
            plan_of(p, B, Hs, Ws, ME, Ms, nlev, ragged != 0);
            printf("L%d %s %s ragged %d: total %zu max_container %zu uniform %d key", nlev, s.name, src.name, ragged, p.total, p.max_container, p.uniform ? 1 : 0);
            for (long k : p.key) printf(" %ld", k);
            printf("\n");
        }
    for (const Modes &t : targets)
        printf("L%d %s %s -> %s: transcode workspace %zu\n", nlev, s.name, src.name, t.name,
               plan_transcode_workspace_bytes(B, Hs, Ws, src.m.data(), (int)src.m.size(), t.m.data(), (int)t.m.size(), nlev));
}

static void queries()
{
    const Sizes one32{ "1x32x32", { 32 }, { 32 } }, one96{ "1x96x160", { 96 }, { 160 } }, three32{ "3x32x32", { 32, 32, 32 }, { 32, 32, 32 } },
                three96{ "3x96x160", { 96, 96, 96 }, { 160, 160, 160 } }, mixed{ "96x160+67x93+32x33", { 96, 67, 32 }, { 160, 93, 33 } },
                small{ "96x160+31x93+32x33", { 96, 31, 32 }, { 160, 93, 33 } };
    const Modes m_ac{ "ac", { ac } }, m_r8{ "rans8", { r8 } }, m_w14{ "wide14", { w14 } }, m_x64{ "xwide64", { x64 } }, m_xa3{ "xauto3", { xa3 } }, m_x8{ "xwide8", { x8 } },
                m_bad{ "unknown", { bad } };
    // one mode per image (B = 3)
    const Modes pi_equal{ "[x8 x8 x8]", { x8, x8, x8 } }, pi_count{ "[x4 x8 x16]", { x4, x8, x16 } }, pi_auto{ "[x4 xauto3 x8]", { x4, xa3, x8 } },
                pi_all_auto{ "[xauto3 xauto3 xauto3]", { xa3, xa3, xa3 } }, pi_narrow{ "[r8 r8 r8]", { r8, r8, r8 } }, pi_ac{ "[ac ac ac]", { ac, ac, ac } },
                pi_kinds{ "[x4 rans8 x4]", { x4, r8, x4 } }, pi_ac_x{ "[ac x4 ac]", { ac, x4, ac } }, pi_bad{ "[x4 unknown x4]", { x4, bad, x4 } },
                pi_two{ "[x4 x8]", { x4, x8 } };
    const std::vector<Modes> targets = { m_ac, m_x8, m_xa3 }, targets3 = { m_ac, m_x8, m_xa3, pi_auto, pi_kinds, pi_bad, pi_two };
    for (const Sizes *s : { &one32, &one96, &three32, &three96, &mixed }) {
        const bool three = s->Hs.size() == 3;
        for (const Modes *m : { &m_ac, &m_r8, &m_w14, &m_x64, &m_xa3, &m_bad }) query(*s, *m, three ? targets3 : targets, LLICTI_NLEVELS);
        if (three)
            for (const Modes *m : { &pi_equal, &pi_count, &pi_auto, &pi_all_auto, &pi_narrow, &pi_ac, &pi_kinds, &pi_ac_x, &pi_bad, &pi_two })
                query(*s, *m, targets3, LLICTI_NLEVELS);
    }
    query(small, m_x8, targets, LLICTI_NLEVELS);       // an image below 32 pixels: every query refuses
    query(one96, pi_equal, targets, LLICTI_NLEVELS);   // three modes for one image
    // config B (2 levels): the reference format and xwide streams, at most 18 per image; header grids of at most 255 per side
    const Modes m_x18{ "xwide18", { x18 } }, m_x19{ "xwide19", { x19 } }, m_xa10{ "xauto10", { xa10 } }, pi_b{ "[x4 x18 xauto3]", { x4, x18, xa3 } },
                pi_b19{ "[x4 x19 x8]", { x4, x19, x8 } };
    const Sizes wide_b{ "1x1024x32", { 1024 }, { 32 } }, tall_b{ "1x32x1024", { 32 }, { 1024 } }, fits_b{ "1x1020x32", { 1020 }, { 32 } };
    const std::vector<Modes> targets_b = { m_ac, m_x18, m_x19, m_xa3, m_xa10, m_r8 };
    for (const Sizes *s : { &one32, &one96, &three96, &mixed, &wide_b, &tall_b, &fits_b })
        for (const Modes *m : { &m_ac, &m_x18, &m_x19, &m_r8, &m_w14, &m_xa3, &m_xa10 }) query(*s, *m, targets_b, kLevelsB);
    query(three96, pi_b, { m_ac, pi_b, pi_b19 }, kLevelsB);
    query(mixed, pi_b19, { m_x18 }, kLevelsB);
    for (int nlev : { LLICTI_NLEVELS, kLevelsB })
        for (const auto &hw : { std::pair<int, int>{ 32, 32 }, { 96, 160 }, { 67, 93 }, { 32, 33 }, { 1024, 32 }, { 31, 64 }, { 64, 8161 } })
            printf("L%d %dx%d: max container %zu\n", nlev, hw.first, hw.second, plan_max_container_bytes(hw.first, hw.second, nlev));
}

// The bound on a stream's bits (check_stream_bits): a slot of 2^28 bytes or more is refused.  The boundary is FOUND with the rule and then held
// against the plan builder's own slot size and against the 32-bit bit position the rule protects; the heights go to stdout, into the recorded answers.
static bool admits(int H, int W, int mode, int nlev = LLICTI_NLEVELS)
{
    const int ME = mode_streams(mode);
    return check_dims(1, H, W) == 0 && check_stream_bits("encode_images", nlev, 1, &H, &W, ME, {}) == 0;
}
static long slot_of(int H, int W, int mode)
{
    Plan p;
    build_plan(p, PlanSpec{ 1, &H, &W, mode_streams(mode), nullptr, LLICTI_NLEVELS, false });
    return p.rslot_cap;
}
static void stream_bits()
{
    const int W = 8160;
    const struct { const char *name; int base; } kinds[3] = { { "rans", 0x100 }, { "wide", 0x300 }, { "xwide", 0x500 } };
    for (const auto &k : kinds) {
        const int one = k.base | 1, two = k.base | 2;
        // the largest image: refused in one stream, admitted in two -- by the rule, the size queries and both sides of a transcode
        REQUIRE(!admits(8160, 8160, one) && admits(8160, 8160, two));
        const int H8 = 8160;
        g_err.clear();
        REQUIRE(plan_workspace_bytes(1, 8160, 8160, one) == 0 && g_err.find("image 0 is 8160x8160") != std::string::npos);
        REQUIRE(g_err.find("in 1 stream ") != std::string::npos && g_err.find("the smallest count that fits is 2") != std::string::npos);
        REQUIRE(plan_workspace_bytes(1, 8160, 8160, two) > 0 && plan_workspace_bytes_v(1, &H8, &H8, one) == 0 && plan_workspace_bytes_vm(1, &H8, &H8, &one, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(1, &H8, &H8, &one, 1, &two, 1) == 0 && plan_transcode_workspace_bytes(1, &H8, &H8, &two, 1, &one, 1) == 0);
        REQUIRE(plan_transcode_workspace_bytes(1, &H8, &H8, &two, 1, &two, 1) > 0 && plan_transcode_workspace_bytes(1, &H8, &H8, &ac, 1, &two, 1) > 0);
        // the exact boundary at W = 8160: the largest H one stream still takes
        int H = 32;
        while (H < 8160 && admits(H + 1, W, one)) ++H;
        REQUIRE(H < 8160 && admits(H, W, one) && !admits(H + 1, W, one));
        for (int h = H + 1; h <= 8160; h += 97) REQUIRE(!admits(h, W, one));                      // (monotone: nothing above it slips through)
        const long fits = slot_of(H, W, one), over = slot_of(H + 1, W, one);
        REQUIRE(fits < (1L << 28) && over >= (1L << 28));                                          // the plan's own slot, on either side of 2^28 bytes
        REQUIRE(8 * fits <= 0x7FFFFFFFL && 8 * over > 0x7FFFFFFFL);                                // ... which is where the bit position leaves a signed int
        REQUIRE(plan_workspace_bytes(1, H, W, one) > 0 && plan_workspace_bytes(1, H + 1, W, one) == 0 && plan_workspace_bytes(1, H + 1, W, two) > 0);
        printf("stream bits %s: 8160x8160 refused in 1 stream, admitted in 2; W=8160, 1 stream: H=%d admitted (slot %ld), H=%d refused (slot %ld)\n", k.name, H, fits, H + 1, over);
    }
    // an "auto" image is bounded at the fewest streams its encoder may pick: size rule 2 -> 1 .. 3 streams
    REQUIRE(!admits(8160, 8160, LLICTI_MODE_RANS_X_AUTO(2)) && !admits(8160, 8160, LLICTI_MODE_RANS_X_AUTO(1)) && admits(8160, 8160, LLICTI_MODE_RANS_X_AUTO(3)));
    // one image of a batch is enough, and the message names it; per-image modes are read per image
    const int Hs[3] = { 96, 8160, 64 }, Ws[3] = { 160, 8160, 64 };
    const int x1 = LLICTI_MODE_RANS_X(1), per_ok[3] = { x1, x4, x1 }, per_bad[3] = { x4, x1, x4 };
    int ME = 0;
    std::vector<int> Ms;
    g_err.clear();
    REQUIRE(plan_workspace_bytes_v(3, Hs, Ws, x1) == 0 && g_err.find("image 1 is 8160x8160") != std::string::npos);
    REQUIRE(plan_workspace_bytes_vm(3, Hs, Ws, per_ok, 3) > 0 && plan_workspace_bytes_vm(3, Hs, Ws, per_bad, 3) == 0);
    REQUIRE(resolve_modes("decode_images", per_bad, 3, 3, &ME, Ms) == 0 && check_stream_bits("decode_images", LLICTI_NLEVELS, 3, Hs, Ws, ME, Ms) == LLICTI_EINVAL);
    REQUIRE(g_err.compare(0, 15, "decode_images: ") == 0);
    // the reference format has no rANS stream; config B's two levels hold 3/4 of the symbols: the same rule, its own boundary (its header admits at most 1020 pixels a side anyway)
    REQUIRE(admits(8160, 8160, ac) && admits(1020, 1020, x1, kLevelsB));
}

// One faulty input per admission rule: the code, and the caller's prefix in front of the reason.
static bool refused(int rc, const char *who)
{
    const std::string want = std::string(who) + ": ";
    return rc == LLICTI_EINVAL && g_err.compare(0, want.size(), want) == 0;
}
static void refusals()
{
    const int H3[3] = { 96, 96, 96 }, W3[3] = { 160, 160, 160 }, Hm[3] = { 96, 67, 32 }, Wm[3] = { 160, 93, 33 };
    int ME = 0;
    std::vector<int> Ms;
    // the modes of one side
    const int two[2] = { x4, x8 }, kinds[3] = { x4, r8, x4 }, ac_x[3] = { ac, x4, ac }, bad3[3] = { x4, bad, x4 }, counts[3] = { x4, x8, x16 }, mix[3] = { x4, xa3, x8 };
    REQUIRE(refused(resolve_modes("encode_images", nullptr, 1, 3, &ME, Ms), "encode_images"));
    REQUIRE(refused(resolve_modes("encode_images", two, 2, 3, &ME, Ms), "encode_images"));
    REQUIRE(refused(resolve_modes("decode_images", &bad, 1, 3, &ME, Ms), "decode_images"));
    REQUIRE(refused(resolve_modes("decode_images", bad3, 3, 3, &ME, Ms), "decode_images"));
    REQUIRE(refused(resolve_modes("transcode_images (source)", kinds, 3, 3, &ME, Ms), "transcode_images (source)"));
    REQUIRE(refused(resolve_modes("transcode_images (target)", ac_x, 3, 3, &ME, Ms), "transcode_images (target)"));
    REQUIRE(resolve_modes("encode_images", counts, 3, 3, &ME, Ms) == 0 && ME == (4 | 0x200) && Ms == std::vector<int>({ 4, 8, 16 }));
    REQUIRE(resolve_modes("encode_images", mix, 3, 3, &ME, Ms) == 0 && ME == (4 | 0x200 | 0x1000) && Ms == std::vector<int>({ 4, 3 | 0x1000, 8 }));
    const int same[3] = { x8, x8, x8 };
    REQUIRE(resolve_modes("encode_images", same, 3, 3, &ME, Ms) == 0 && ME == (8 | 0x200) && Ms.empty());
    // the modes a model takes: config B refuses narrow and wide streams, more than 18 xwide streams, an "auto" rule above 13
    REQUIRE(check_model(LLICTI_NLEVELS, "encode_images", 128 | 0x200, {}) == 0 && check_model(kLevelsB, "encode_images", 18 | 0x200, {}) == 0);
    REQUIRE(refused(check_model(kLevelsB, "encode_images", 8, {}), "encode_images"));
    REQUIRE(refused(check_model(kLevelsB, "decode_images", 14 | 0x100, {}), "decode_images"));
    REQUIRE(refused(check_model(kLevelsB, "transcode_images (target)", 19 | 0x200, {}), "transcode_images (target)"));
    REQUIRE(refused(check_model(kLevelsB, "transcode_images (source)", 4 | 0x200, { 4, 19, 8 }), "transcode_images (source)"));
    REQUIRE(refused(check_model(kLevelsB, "encode_images", 14 | 0x200 | 0x1000, {}), "encode_images"));
    // "auto" names no container
    REQUIRE(check_source_modes("decode_images", "container", 8 | 0x200) == 0);
    REQUIRE(refused(check_source_modes("decode_images", "container", 3 | 0x200 | 0x1000), "decode_images"));
    REQUIRE(resolve_modes("transcode_images (source)", mix, 3, 3, &ME, Ms) == 0 && refused(check_source_modes("transcode_images", "source container", ME), "transcode_images"));
    // config B's header: the last level's grid in one byte per side
    const int Hb[2] = { 64, 1024 }, Wb[2] = { 48, 32 }, Hok[2] = { 64, 1020 };
    REQUIRE(check_header_grid("encode_images", LLICTI_NLEVELS, 2, Hb, Wb) == 0 && check_header_grid("encode_images", kLevelsB, 2, Hok, Wb) == 0);
    REQUIRE(refused(check_header_grid("encode_images", kLevelsB, 2, Hb, Wb), "encode_images"));
    REQUIRE(refused(check_header_grid("transcode_images", kLevelsB, 2, Wb, Hb), "transcode_images"));
    // a container slot holds at least its image's header: 17 + 3 h w of the last level's grid (96x160, 5 levels: 3 x 5; 2 levels: 24 x 40)
    REQUIRE(header_bytes(96, 160, LLICTI_NLEVELS) == 17 + 3 * 3 * 5 && header_bytes(96, 160, kLevelsB) == 17 + 3 * 24 * 40);
    REQUIRE(check_in_stride("decode_images", LLICTI_NLEVELS, 3, Hm, Wm, 62) == 0);
    REQUIRE(refused(check_in_stride("decode_images", LLICTI_NLEVELS, 3, Hm, Wm, 61), "decode_images"));
    REQUIRE(refused(check_in_stride("transcode_images", kLevelsB, 3, H3, W3, 2896), "transcode_images"));
    // a transcode of mixed sizes (or of force_ragged's placement) needs rANS containers on both sides
    REQUIRE(check_transcode_sizes("transcode_images", 3, Hm, Wm, 8 | 0x200, 4, false) == 0 && check_transcode_sizes("transcode_images", 3, H3, W3, 0, 0, false) == 0);
    REQUIRE(refused(check_transcode_sizes("transcode_images", 3, Hm, Wm, 0, 8 | 0x200, false), "transcode_images"));
    REQUIRE(refused(check_transcode_sizes("transcode_images", 3, Hm, Wm, 8 | 0x200, 0, false), "transcode_images"));
    REQUIRE(refused(check_transcode_sizes("transcode_images", 3, H3, W3, 0, 8 | 0x200, true), "transcode_images"));
    // a size query that refuses leaves the reason behind
    g_err.clear();
    REQUIRE(plan_workspace_bytes_vm(3, H3, W3, kinds, 3) == 0 && !g_err.empty());
    g_err.clear();
    REQUIRE(plan_transcode_workspace_bytes(3, H3, W3, &xa3, 1, &x8, 1) == 0 && !g_err.empty());
}

int main()
{
    queries();
    stream_bits();
    refusals();
    return 0;
}
