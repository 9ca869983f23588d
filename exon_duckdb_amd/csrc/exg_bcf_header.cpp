// exg_bcf_header.cpp — see exg_bcf_header.hpp (host only, no HIP call).
#include "exg_bcf_header.hpp"

#include <string.h>

#include <map>

namespace exg_rd {

int64_t BcfDict::find(const std::string &id) const {
    for (uint32_t i = 0; i < size(); i++)
        if (table[2 * i + 1] == id.size() && bytes.compare(table[2 * i], id.size(), id) == 0) return i;
    return -1;
}

namespace {

// the value of attribute `key` of a structured line's <...> (s = what follows '<'); false: not there.  Values may be quoted
// (a Description with commas in it) and quotes escaped with a backslash
bool attribute(const std::string &s, const char *key, std::string *out) {
    size_t i = 0;
    const size_t klen = strlen(key);
    while (i < s.size() && s[i] != '>') {
        const size_t k0 = i;
        while (i < s.size() && s[i] != '=' && s[i] != ',' && s[i] != '>') i++;
        const bool match = i - k0 == klen && s.compare(k0, klen, key) == 0;
        if (i >= s.size() || s[i] != '=') {  // a key without a value
            if (i < s.size() && s[i] == ',') i++;
            continue;
        }
        i++;
        std::string v;
        if (i < s.size() && s[i] == '"') {
            for (i++; i < s.size() && s[i] != '"'; i++) {
                if (s[i] == '\\' && i + 1 < s.size()) i++;
                v.push_back(s[i]);
            }
            if (i < s.size()) i++;
            while (i < s.size() && s[i] != ',' && s[i] != '>') i++;
        } else {
            while (i < s.size() && s[i] != ',' && s[i] != '>') v.push_back(s[i++]);
        }
        if (match) {
            *out = v;
            return true;
        }
        if (i < s.size() && s[i] == ',') i++;
    }
    return false;
}

struct DictBuilder {
    std::map<std::string, uint32_t> index;
    uint32_t next = 0;
    void add(const std::string &id, const std::string *idx) {
        if (index.count(id)) return;  // (INFO and FORMAT share an ID: one index, the first one's)
        uint32_t at = next;
        if (idx) at = (uint32_t)strtoul(idx->c_str(), nullptr, 10);
        if (at > (1u << 24)) return;  // (an IDX no record can mean: typed keys hold 32 bits, a table that size is nonsense)
        index[id] = at;
        if (at + 1 > next) next = at + 1;
    }
    void finish(BcfDict *d) const {
        d->bytes.clear();
        d->table.assign((size_t)next * 2, 0);
        for (uint32_t i = 0; i < next; i++) d->table[2 * i + 1] = kBcfNoEntry;
        for (const auto &kv : index) {  // (two IDs given one IDX: the greater name stays — no file does that)
            d->table[2 * kv.second] = (uint32_t)d->bytes.size();
            d->table[2 * kv.second + 1] = (uint32_t)kv.first.size();
            d->bytes += kv.first;
        }
    }
};

}  // namespace

int bcf_parse_header(const uint8_t *p, uint64_t n, bool eof, BcfHeader *out, uint64_t *need, std::string *err) {
    *need = 0;
    if (n < 9) {
        if (!eof) {
            *need = 9;
            return kBcfHeaderMore;
        }
        *err = "not a BCF file: the decoded stream is shorter than the magic and the header's length";
        return kBcfHeaderBad;
    }
    if (memcmp(p, "BCF\2", 4) != 0) {
        *err = "not a BCF file: the decoded stream does not begin with the magic BCF\\2\\2";
        return kBcfHeaderBad;
    }
    if (p[4] != 2) {
        *err = "BCF version 2." + std::to_string((unsigned)p[4]) + " is not supported (2.2 is)";
        return kBcfHeaderBad;
    }
    const uint64_t l_text = (uint64_t)p[5] | ((uint64_t)p[6] << 8) | ((uint64_t)p[7] << 16) | ((uint64_t)p[8] << 24);
    if (9 + l_text > n) {
        if (!eof) {
            *need = 9 + l_text;
            return kBcfHeaderMore;
        }
        *err = "truncated BCF header: its text is " + std::to_string(l_text) + " bytes, the stream ends before that";
        return kBcfHeaderBad;
    }
    if (l_text == 0 || p[9 + l_text - 1] != 0) {
        *err = "invalid BCF header: its text is not NUL-terminated";
        return kBcfHeaderBad;
    }
    const char *t = (const char *)p + 9;
    BcfHeader h;
    h.text.assign(t, strnlen(t, (size_t)l_text));
    if (h.text.empty() || h.text.back() != '\n') h.text.push_back('\n');
    h.end = 9 + l_text;
    DictBuilder strings, contigs;
    const std::string pass = "PASS", zero = "0";
    strings.add(pass, &zero);
    bool chrom = false;
    for (size_t pos = 0; pos < h.text.size();) {
        const size_t nl = h.text.find('\n', pos);
        const std::string line = h.text.substr(pos, nl - pos);
        pos = nl + 1;
        const bool filter = line.compare(0, 10, "##FILTER=<") == 0, info = line.compare(0, 8, "##INFO=<") == 0,
                   format = line.compare(0, 10, "##FORMAT=<") == 0, contig = line.compare(0, 10, "##contig=<") == 0;
        if (filter || info || format || contig) {
            const std::string body = line.substr(line.find('<') + 1);
            std::string id, idx;
            if (!attribute(body, "ID", &id)) continue;
            const bool has_idx = attribute(body, "IDX", &idx);
            (contig ? contigs : strings).add(id, has_idx ? &idx : nullptr);
        } else if (line.compare(0, 6, "#CHROM") == 0) {
            chrom = true;
            size_t fields = 1;
            for (char c : line) fields += c == '\t';
            h.n_samples = fields > 9 ? (uint32_t)(fields - 9) : 0;
            break;
        }
    }
    if (!chrom) {
        *err = "invalid BCF header: no #CHROM line";
        return kBcfHeaderBad;
    }
    strings.finish(&h.strings);
    contigs.finish(&h.contigs);
    const int64_t gt = h.strings.find("GT");
    h.gt_index = gt < 0 ? ~0u : (uint32_t)gt;
    *out = h;
    return kBcfHeaderOk;
}

}  // namespace exg_rd
