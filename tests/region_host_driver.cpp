// tests/region_host_driver.cpp — TEST INFRASTRUCTURE: a stand-alone program (its own main, no Python, no GPU) over the host side of
// vcf_query — the tabix parser, the region grammar and the planner of csrc/exg_tabix.cpp, through exg_tabix_query where a caller
// would go through it, and the host compile of the predicate's rules (csrc/exg_vcf_region.hpp, the code the device kernel runs) —
// built with AddressSanitizer + UBSan (tests/test_region_host.py builds and runs it).  Every index and every field lives in a heap
// block of EXACTLY its length, so a read one byte in front of it or behind it is a report.
//
// usage: region_host_driver <inflated .tbi> ...   per index: the plan of every name (printed, so that the caller can hold it
// against its own planner), every truncation, every aligned word overwritten with a huge and a negative count
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "exg_tabix.cpp"
#include "exg_vcf_region.hpp"

namespace exg {
static std::string g_error;
void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace exg

namespace tb = exg::tabix;
namespace vr = exg::vcf_region;

static int g_fail = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                         \
        }                                                                     \
    } while (0)

struct Exact {  // a heap copy of exactly n bytes
    uint8_t *p;
    size_t n;
    Exact(const void *d, size_t len) : p((uint8_t *)malloc(len ? len : 1)), n(len) {
        if (len) memcpy(p, d, len);
    }
    explicit Exact(const std::string &s) : Exact(s.data(), s.size()) {}
    ~Exact() { free(p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
};

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33) % n;
}

// exg_tabix_query by its two-call protocol on an exactly-sized copy of the index
static int query(const Exact &idx, const std::string &region, std::vector<exg_virtual_chunk> *chunks, exg_region *resolved) {
    uint64_t n = 0;
    chunks->clear();
    int rc = exg_tabix_query(idx.p, idx.n, region.c_str(), nullptr, 0, &n, resolved);
    if (rc) return rc;
    std::vector<exg_virtual_chunk> out(n + 1, exg_virtual_chunk{0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull});
    uint64_t n2 = 0;
    rc = exg_tabix_query(idx.p, idx.n, region.c_str(), out.data(), n, &n2, resolved);
    CHECK(rc == EXG_OK && n2 == n && out[n].begin == 0xA5A5A5A5A5A5A5A5ull);
    if (n > 0) {  // one short: EXG_E_CAPACITY, the count still told, nothing written
        std::vector<exg_virtual_chunk> small(n, exg_virtual_chunk{7, 7});
        uint64_t n3 = 0;
        CHECK(exg_tabix_query(idx.p, idx.n, region.c_str(), small.data(), n - 1, &n3, nullptr) == EXG_E_CAPACITY && n3 == n && small[0].begin == 7);
    }
    out.resize(n);
    *chunks = out;
    return EXG_OK;
}

static uint64_t g_plans = 0, g_truncations = 0, g_overwrites = 0;

static void one_index(const char *path) {
    std::ifstream f(path, std::ios::binary);
    const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    CHECK(!bytes.empty());
    const Exact whole(bytes);
    tb::Index idx;
    std::string err;
    CHECK(tb::parse_index(whole.p, whole.n, &idx, &err));
    if (g_fail) return;
    // the plan of every name, unbounded and in windows; the pseudo-bin never shows
    for (size_t i = 0; i < idx.refs.size(); i++) {
        for (const tb::Bin &b : idx.refs[i].bins)
            if (b.id == tb::kPseudoBin) CHECK(b.n_chunks == 2);
        std::vector<std::string> regions = {idx.refs[i].name};
        for (int k = 0; k < 8; k++) {
            const uint64_t s = 1 + (k < 4 ? rnd(1u << 21) : 16384u * (1 + rnd(127)) - rnd(2));  // (anywhere, and at the 16 KiB windows' edges)
            regions.push_back(idx.refs[i].name + ":" + std::to_string(s) + "-" + std::to_string(s + rnd(1u << 16)));
            regions.push_back(idx.refs[i].name + ":" + std::to_string(s));
        }
        for (const std::string &r : regions) {
            std::vector<exg_virtual_chunk> chunks;
            exg_region res;
            CHECK(query(whole, r, &chunks, &res) == EXG_OK);
            CHECK(res.ref_id == i && std::string(res.name, res.name_len) == idx.refs[i].name && res.start >= 1 && res.end >= res.start);
            printf("plan %s %s", path, r.c_str());
            for (size_t k = 0; k < chunks.size(); k++) {
                CHECK(chunks[k].begin < chunks[k].end && (!k || chunks[k - 1].end < chunks[k].begin));
                printf(" %llx-%llx", (unsigned long long)chunks[k].begin, (unsigned long long)chunks[k].end);
            }
            printf("\n");
            g_plans++;
        }
    }
    // every truncation fails — except the one that drops exactly the optional n_no_coor, which gives the same plans
    for (size_t n = 0; n < whole.n; n++) {
        const Exact cut(whole.p, n);
        tb::Index t;
        const bool ok = tb::parse_index(cut.p, cut.n, &t, &err);
        if (idx.has_no_coor && n == whole.n - 8) {
            CHECK(ok && !t.has_no_coor && t.refs.size() == idx.refs.size());
        } else {
            CHECK(!ok && !err.empty());
            uint64_t k = 0;
            CHECK(exg_tabix_query(cut.p, cut.n, idx.refs.empty() ? "x" : idx.refs[0].name.c_str(), nullptr, 0, &k, nullptr) == EXG_E_PARSE);
        }
        g_truncations++;
        if (whole.n > 4096 && n > 512 && n + 512 < whole.n) n += rnd(7);  // (a long index: every byte at both ends, a stride between)
    }
    // every aligned word as a huge count and as a negative one: an error or an index, never a read outside the block
    for (size_t at = 4; at + 4 <= whole.n; at += 4) {
        for (uint32_t v : {0x7FFFFFFFu, 0xFFFFFFFFu, 0x01000000u}) {
            Exact bad(whole.p, whole.n);
            memcpy(bad.p + at, &v, 4);
            tb::Index t;
            if (tb::parse_index(bad.p, bad.n, &t, &err))
                for (size_t i = 0; i < t.refs.size(); i++) {
                    std::vector<exg_virtual_chunk> chunks;
                    tb::Region reg;
                    reg.ref_id = (uint32_t)i, reg.start = 1 + rnd(1u << 22), reg.end = reg.start + rnd(1u << 20);
                    tb::plan(t, reg, &chunks);
                }
            g_overwrites++;
        }
        if (whole.n > 4096 && at > 512 && at + 512 < whole.n) at += 4 * rnd(5);
    }
}

// ---- the grammar, on a hand-made index --------------------------------------------------------------------------------------
static std::string tiny_index(const std::vector<std::string> &names) {
    std::string nm;
    for (const std::string &n : names) nm += n, nm.push_back('\0');
    std::string out("TBI\1", 4);
    auto i32 = [&](int32_t v) { out.append((const char *)&v, 4); };
    auto u64 = [&](uint64_t v) { out.append((const char *)&v, 8); };
    i32((int32_t)names.size()), i32(2), i32(1), i32(2), i32(0), i32('#'), i32(0), i32((int32_t)nm.size());
    out += nm;
    for (size_t i = 0; i < names.size(); i++) {
        i32(2);
        i32(4681), i32(1), u64(0x10000 * (i + 1)), u64(0x10000 * (i + 1) + 0x80);
        i32((int32_t)tb::kPseudoBin), i32(2), u64(1), u64(2), u64(3), u64(0);
        i32(1), u64(0x10000 * (i + 1));
    }
    u64(0);
    return out;
}

static void grammar() {
    const Exact idx(tiny_index({"1", "10", "chr1:5", "HLA-A*01:01", "a:b:7-9"}));
    struct Case {
        const char *text;
        int rc;
        const char *name;
        int64_t start, end;
    } cases[] = {
        {"1", EXG_OK, "1", 1, tb::kUnbounded},                    // G1
        {"10", EXG_OK, "10", 1, tb::kUnbounded},                  // (`1` is not `10`)
        {"1:5", EXG_OK, "1", 5, tb::kUnbounded},                  // G2 name:start
        {"1:5-9", EXG_OK, "1", 5, 9},                             // G2 name:start-end
        {"1:5-5", EXG_OK, "1", 5, 5},
        {"chr1:5", EXG_OK, "chr1:5", 1, tb::kUnbounded},          // G1 wins over the split
        {"chr1:5:7", EXG_OK, "chr1:5", 7, tb::kUnbounded},        // the LAST colon
        {"chr1:5:7-8", EXG_OK, "chr1:5", 7, 8},
        {"HLA-A*01:01", EXG_OK, "HLA-A*01:01", 1, tb::kUnbounded},
        {"HLA-A*01:01:100-200", EXG_OK, "HLA-A*01:01", 100, 200},
        {"a:b:7-9", EXG_OK, "a:b:7-9", 1, tb::kUnbounded},        // a name that looks like an interval at its end
        {"a:b:7-9:3", EXG_OK, "a:b:7-9", 3, tb::kUnbounded},
        {"", EXG_E_INVALID_ARG, "", 0, 0},                        // G5
        {"2", EXG_E_INVALID_ARG, "", 0, 0},
        {"2:5", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:0", EXG_E_INVALID_ARG, "", 0, 0},                     // start >= 1: no interval, the whole string is the name
        {"1:9-5", EXG_E_INVALID_ARG, "", 0, 0},                   // end >= start
        {"1:5-", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:-5", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:1,000", EXG_E_INVALID_ARG, "", 0, 0},                 // digits only
        {"1:+5", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:5 ", EXG_E_INVALID_ARG, "", 0, 0},
        {"1:1234567890123456789", EXG_E_INVALID_ARG, "", 0, 0},   // 19 digits
        {":5", EXG_E_INVALID_ARG, "", 0, 0},
        {"1 ", EXG_E_INVALID_ARG, "", 0, 0},
    };
    for (const Case &c : cases) {
        const Exact text(c.text, strlen(c.text) + 1);
        exg_region res;
        uint64_t n = 0;
        const int rc = exg_tabix_query(idx.p, idx.n, (const char *)text.p, nullptr, 0, &n, &res);
        CHECK(rc == c.rc);
        if (rc != c.rc) fprintf(stderr, "  region '%s': rc %d, want %d\n", c.text, rc, c.rc);
        if (rc == EXG_OK) CHECK(std::string(res.name, res.name_len) == c.name && res.start == c.start && res.end == c.end && n == 1);
        else CHECK(exg::g_error.find(std::string("'") + c.text + "'") != std::string::npos);  // the error names the region
    }
    // format != 2 is refused
    std::string sam = tiny_index({"1"});
    const int32_t one = 1;
    sam.replace(8, 4, (const char *)&one, 4);
    const Exact sam_idx(sam);
    uint64_t n = 0;
    CHECK(exg_tabix_query(sam_idx.p, sam_idx.n, "1", nullptr, 0, &n, nullptr) == EXG_E_PARSE && exg::g_error.find("format") != std::string::npos);
}

// ---- the predicate's rules ------------------------------------------------------------------------------------------------
// the same question asked the slow way: split at `;`, the first item that is END or begins with END=
static bool slow_info_end(const std::string &info, int64_t *out) {
    for (size_t i = 0; i <= info.size();) {
        size_t e = info.find(';', i);
        if (e == std::string::npos) e = info.size();
        const std::string item = info.substr(i, e - i);
        if (item == "END") return false;
        if (item.compare(0, 4, "END=") == 0) {
            const std::string v = item.substr(4);
            if (v.empty() || v.size() > 18) return false;
            int64_t x = 0;
            for (char ch : v) {
                if (ch < '0' || ch > '9') return false;
                x = x * 10 + (ch - '0');
            }
            *out = x;
            return true;
        }
        i = e + 1;
    }
    return false;
}

static uint64_t g_infos = 0;
static void info_case(const std::string &info) {
    const Exact e(info);
    int64_t a = -1, b = -1;
    const bool fa = vr::info_end(e.p, (uint32_t)e.n, &a), fb = slow_info_end(info, &b);
    CHECK(fa == fb && (!fa || a == b));
    if (fa != fb || (fa && a != b)) fprintf(stderr, "  INFO '%s': %d %lld, want %d %lld\n", info.c_str(), fa, (long long)a, fb, (long long)b);
    g_infos++;
}

static void predicate() {
    int64_t v = 0;
    auto end_of = [&](const char *s) {
        const Exact e(s, strlen(s));
        v = -1;
        return vr::info_end(e.p, (uint32_t)e.n, &v) ? v : -1;
    };
    CHECK(end_of("END=5") == 5 && end_of("X=1;END=5") == 5 && end_of("SVEND=9;END=5") == 5 && end_of("DP=1;END=5;X") == 5);
    CHECK(end_of("END") == -1 && end_of("END=.") == -1 && end_of("END=") == -1 && end_of(".") == -1 && end_of("") == -1);
    CHECK(end_of("SVEND=9") == -1 && end_of("END=5x") == -1 && end_of("END=-5") == -1 && end_of("ENDX=5") == -1 && end_of("XEND=5") == -1);
    CHECK(end_of("END;END=5") == -1 && end_of("END=.;END=5") == -1 && end_of("END=5;END=9") == 5 && end_of("EN") == -1 && end_of(";END=7") == 7);
    CHECK(end_of("END=123456789012345678") == 123456789012345678ll && end_of("END=1234567890123456789") == -1);
    const char *alphabet[] = {"END", "END=", "SVEND=", "DP=", ";", ";", "=", "5", "17", ".", "E", "N", "D", "x", "END=12", ";END"};
    for (int it = 0; it < 20000; it++) {
        std::string s;
        for (uint32_t k = rnd(7); k; k--) s += alphabet[rnd(sizeof alphabet / sizeof *alphabet)];
        info_case(s);
    }
    // R1: the lengths are equal too
    const Exact one("1"), ten("10"), chr("chr1"), chs("chr2");
    CHECK(vr::same_name(one.p, 1, one.p, 1) && !vr::same_name(one.p, 1, ten.p, 2) && !vr::same_name(ten.p, 2, one.p, 1));
    CHECK(!vr::same_name(chr.p, 4, chs.p, 4) && vr::same_name(chr.p, 4, chr.p, 4));
    // R2 / R3 / E3 / E4: (pos, len(ref), INFO) against [100, 200]
    auto keeps = [&](int64_t pos, uint32_t ref_len, const char *info) {
        const Exact e(info, strlen(info));
        return vr::overlaps(pos, ref_len, e.p, (uint32_t)e.n, 100, 200);
    };
    CHECK(keeps(100, 1, ".") && keeps(200, 1, ".") && !keeps(201, 1, ".") && !keeps(99, 1, "."));
    CHECK(keeps(99, 2, ".") && keeps(1, 100, "DP=1") && !keeps(1, 99, "DP=1"));          // a deletion that reaches in
    CHECK(keeps(50, 1, "END=100") && !keeps(50, 1, "END=99") && keeps(50, 1, "X=1;END=5000"));
    CHECK(!keeps(50, 300, "END=60"));                                                     // END decides, not len(ref)
    CHECK(keeps(50, 300, "END=.") && keeps(50, 300, "END") && !keeps(50, 1, "SVEND=150"));  // absent: len(ref)
    CHECK(keeps(150, 1, "END=120") && !keeps(250, 1, "END=120"));                          // E4: INFO is not looked at
}

int main(int argc, char **argv) {
    grammar();
    predicate();
    for (int i = 1; i < argc; i++) one_index(argv[i]);
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("region host functions ok: %d indexes, %llu plans, %llu truncations, %llu overwritten words, %llu INFO texts\n", argc - 1,
           (unsigned long long)g_plans, (unsigned long long)g_truncations, (unsigned long long)g_overwrites, (unsigned long long)g_infos);
    return 0;
}
