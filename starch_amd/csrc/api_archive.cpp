// starch_amd/csrc/api_archive.cpp -- the archive's index and footer, written and read.
// Host only: nothing here calls HIP.
#include <string.h>

#include <string>
#include <vector>

#include "api_int.hpp"
#include "shard.hpp"

using namespace api;

namespace archive {
const uint8_t kMagic[4] = {0xca, 0x5c, 0xad, 0x1a};   // hpp:907-910
}  // namespace archive

namespace {

bool valid_utf8(const unsigned char* s, size_t n)
{
    for (size_t i = 0; i < n;) {
        unsigned char c = s[i];
        int k = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : -1;
        if (k < 0 || i + k >= n + (k == 0 ? 1 : 0)) return false;
        for (int j = 1; j <= k; ++j) if (i + j >= n || (s[i + j] & 0xc0) != 0x80) return false;
        i += 1 + k;
    }
    return true;
}

}  // namespace

namespace api {

// Chromosome names are arbitrary bytes: escaped byte-wise as \u00XX so the
// original bytes are recovered as latin-1 code points.  Free text (the note)
// that is valid UTF-8 is kept as UTF-8.
void json_str(std::string& o, const char* p, size_t n, bool keep_utf8)
{
    static const char* hx = "0123456789abcdef";
    const bool raw_hi = keep_utf8 && valid_utf8(reinterpret_cast<const unsigned char*>(p), n);
    o += '"';
    for (size_t i = 0; i < n; ++i) {
        unsigned char c = (unsigned char)p[i];
        if (c == '"') o += "\\\"";
        else if (c == '\\') o += "\\\\";
        else if (c >= 0x80 && raw_hi) o += (char)c;
        else if (c < 0x20 || c >= 0x7f) {   // control and non-ASCII bytes as latin-1 code points
            o += "\\u00";
            o += hx[c >> 4];
            o += hx[c & 15];
        } else o += (char)c;
    }
    o += '"';
}

}  // namespace api

std::string archive::build_index(const starch_segment* segs, const char* const* names, const uint64_t* nlens, uint64_t nseg,
                        uint64_t index_off, const char* note, int bs, bool base_counts, int method)
{
    std::string j;
    j += "{\"archive\":{\"type\":\"starch\",\"format\":\"starch3-mi355x\",\"version\":{\"major\":3,\"minor\":0,"
         "\"revision\":0},\"compressionFormat\":";
    j += method == STARCH_METHOD_GZIP ? "\"gzip\",\"blockSize100k\":" : "\"bzip2\",\"blockSize100k\":";
    j += std::to_string(method == STARCH_METHOD_GZIP ? 0 : bs);
    j += ",\"note\":";
    json_str(j, note ? note : "", note ? strlen(note) : 0, true);
    j += "},\"streams\":[";
    for (uint64_t s = 0; s < nseg; ++s) {
        if (s) j += ',';
        j += "{\"chromosome\":";
        json_str(j, names[s], nlens[s]);
        j += ",\"offset\":" + std::to_string(segs[s].stream_offset);
        j += ",\"size\":" + std::to_string(segs[s].stream_bytes);
        j += ",\"uncompressedLineCount\":" + std::to_string(segs[s].line_count);
        j += ",\"transformedBytes\":" + std::to_string(segs[s].text_bytes);
        j += ",\"blocks\":" + std::to_string(segs[s].n_blocks);
        j += ",\"combinedCRC\":" + std::to_string(segs[s].combined_crc);
        if (base_counts) {   // hpp:61-62
            j += ",\"uniqueBaseCount\":" + std::to_string(segs[s].base_count_unique);
            j += ",\"nonUniqueBaseCount\":" + std::to_string(segs[s].base_count_nonunique);
        }
        j += '}';
    }
    j += "]}";
    // 32-byte footer: zero-padded decimal offset of the index, then padding + '\n'
    char foot[40];
    snprintf(foot, sizeof(foot), "%020llu", (unsigned long long)index_off);
    std::string f(foot);
    f.append(31 - f.size(), ' ');
    f += '\n';
    return j + f;
}

std::string api::index_of(const std::vector<starch_segment>& segs, const std::vector<std::string>& names,
                          uint64_t index_off, const starch_options& opt)
{
    std::vector<const char*> np(segs.size());
    std::vector<uint64_t> nl(segs.size());
    for (size_t s = 0; s < segs.size(); ++s) { np[s] = names[s].data(); nl[s] = names[s].size(); }
    return build_index(segs.data(), np.data(), nl.data(), segs.size(), index_off, opt.note, opt.block_size_100k,
                       opt.base_counts != 0, opt.compression_method);
}

namespace {

// JSON string body at j[q] (after the opening quote) up to `end`; q is left on
// the closing quote.  bytewise: \u00XX is one byte (chromosome names), else
// the code point as UTF-8 (the note).
bool json_unescape(const std::string& j, size_t& q, size_t end, bool bytewise, std::string& out)
{
    for (;;) {
        if (q >= end) return false;
        const char ch = j[q];
        if (ch == '"') return true;
        if (ch != '\\') { out += ch; ++q; continue; }
        if (q + 1 >= end) return false;
        const char x = j[q + 1];
        if (x == 'u') {
            if (q + 6 > end) return false;
            unsigned v = 0;
            for (int k = 2; k < 6; ++k) {
                const char h = j[q + k];
                v = v * 16 + (unsigned)(h >= '0' && h <= '9' ? h - '0' : h >= 'a' && h <= 'f' ? h - 'a' + 10
                                         : h >= 'A' && h <= 'F' ? h - 'A' + 10 : 0);
            }
            if (bytewise || v < 0x80) out += (char)v;
            else if (v < 0x800) { out += (char)(0xc0 | (v >> 6)); out += (char)(0x80 | (v & 63)); }
            else { out += (char)(0xe0 | (v >> 12)); out += (char)(0x80 | ((v >> 6) & 63)); out += (char)(0x80 | (v & 63)); }
            q += 6;
        } else {
            out += x == 'n' ? '\n' : x == 't' ? '\t' : x == 'r' ? '\r' : x == 'b' ? '\b' : x == 'f' ? '\f' : x;
            q += 2;
        }
    }
}

}  // namespace

namespace api {

// Reader of this library's archive index (build_index above): the footer's
// index offset, the archive fields, then per stream its chromosome (JSON
// string, \u00XX escapes byte-wise) and every field build_index writes.
// offset and size are required; the other fields are 0 when absent.  Throws
// on a layout build_index does not write.
std::vector<IndexEntry> read_index(const uint8_t* a, uint64_t n, uint64_t* index_off, ArchiveInfo* info)
{
    auto bad = [](const char* m) { throw StarchError(STARCH_ERR_DATA, std::string("archive: ") + m); };
    if (n < 4 + 32 || memcmp(a, kMagic, 4) != 0) bad("no magic / footer");
    const char* f = reinterpret_cast<const char*>(a + n - 32);
    uint64_t off = 0;
    for (int i = 0; i < 20; ++i) {
        if (f[i] < '0' || f[i] > '9') bad("footer");
        off = off * 10 + (uint64_t)(f[i] - '0');
    }
    if (f[31] != '\n' || off < 4 || off > n - 32) bad("footer");
    *index_off = off;
    const std::string j(reinterpret_cast<const char*>(a + off), n - 32 - off);
    std::vector<IndexEntry> out;
    size_t p = j.find("\"streams\":[");
    if (p == std::string::npos) bad("index without streams");
    if (info) {   // the archive object precedes the streams; its note is the last field
        auto str = [&](const char* key, bool bytewise, std::string& dst) {
            const std::string k = std::string("\"") + key + "\":\"";
            size_t q = j.find(k);
            if (q == std::string::npos || q > p) return;
            q += k.size();
            if (!json_unescape(j, q, p, bytewise, dst)) bad("index string");
        };
        str("compressionFormat", true, info->format);
        str("note", false, info->note);
        const size_t q = j.find("\"blockSize100k\":");
        if (q != std::string::npos && q < p) info->block_size_100k = atoi(j.c_str() + q + 16);
    }
    p += 11;
    // from: the end of the entry's chromosome string, so a name's bytes are never taken for a key
    auto find_num = [&](const char* key, size_t from, size_t to, bool need, bool* neg) -> std::pair<bool, uint64_t> {
        const std::string k = std::string("\"") + key + "\":";
        size_t q = j.find(k, from);
        if (q == std::string::npos || q > to) {
            if (need) bad("index field missing");
            return {false, 0};
        }
        q += k.size();
        if (neg) {
            *neg = q < j.size() && j[q] == '-';
            if (*neg) ++q;
        }
        uint64_t v = 0;
        if (q >= j.size() || j[q] < '0' || j[q] > '9') bad("index number");
        while (q < j.size() && j[q] >= '0' && j[q] <= '9') v = v * 10 + (uint64_t)(j[q++] - '0');
        return {true, v};
    };
    while (p < j.size() && j[p] == '{') {
        size_t q = j.find("\"chromosome\":\"", p);
        if (q != p + 1) bad("index chromosome");
        q += 14;
        IndexEntry en;
        if (!json_unescape(j, q, j.size(), true, en.chr)) bad("index string");
        const size_t e = j.find('}', q);   // entries hold no nested objects
        if (e == std::string::npos) bad("index entry");
        en.offset = find_num("offset", q, e, true, nullptr).second;
        en.size = find_num("size", q, e, true, nullptr).second;
        en.line_count = find_num("uncompressedLineCount", q, e, false, nullptr).second;
        en.text_bytes = find_num("transformedBytes", q, e, false, nullptr).second;
        en.n_blocks = (uint32_t)find_num("blocks", q, e, false, nullptr).second;
        en.combined_crc = (uint32_t)find_num("combinedCRC", q, e, false, nullptr).second;
        bool neg = false;
        const auto u = find_num("uniqueBaseCount", q, e, false, &neg);
        if (u.first) {
            en.has_base_counts = true;
            en.base_unique = (int64_t)(neg ? 0ull - u.second : u.second);
            const auto v = find_num("nonUniqueBaseCount", q, e, false, &neg);
            en.base_nonunique = (int64_t)(neg ? 0ull - v.second : v.second);
        }
        out.push_back(en);
        p = e + 1;
        if (p < j.size() && j[p] == ',') ++p;
    }
    return out;
}

// every stream inside [4, index offset)
void check_bounds(const std::vector<IndexEntry>& idx, uint64_t index_off)
{
    for (size_t k = 0; k < idx.size(); ++k)
        if (idx[k].offset < 4 || idx[k].offset > index_off || idx[k].size > index_off - idx[k].offset)
            throw StarchError(STARCH_ERR_DATA, "archive: stream " + std::to_string(k) + " lies outside the stream region");
}

}  // namespace api

// the built index to the caller: its length always, its bytes when dst is given
static int index_out(const std::string& s, char* dst, uint64_t cap, uint64_t* len)
{
    *len = s.size();
    if (!dst) return STARCH_OK;
    if (cap < s.size()) return STARCH_ERR_MEM;
    memcpy(dst, s.data(), s.size());
    return STARCH_OK;
}

extern "C" {

int starch_build_index(const starch_segment* segs, const char* const* names, const uint64_t* name_lens,
                       uint64_t nseg, uint64_t index_offset, const char* note, int bs, char* dst, uint64_t cap,
                       uint64_t* len)
{
    if (!len || (nseg && (!segs || !names || !name_lens))) return STARCH_ERR_ARG;
    std::string s = build_index(segs, names, name_lens, nseg, index_offset, note, bs);
    return index_out(s, dst, cap, len);
}

int starch_build_index_opt(const starch_segment* segs, const char* const* names, const uint64_t* name_lens,
                           uint64_t nseg, uint64_t index_offset, const starch_options* opt, char* dst, uint64_t cap,
                           uint64_t* len)
{
    if (!len || !opt || (nseg && (!segs || !names || !name_lens))) return STARCH_ERR_ARG;
    std::string s = build_index(segs, names, name_lens, nseg, index_offset, opt->note, opt->block_size_100k,
                                opt->base_counts != 0, opt->compression_method);
    return index_out(s, dst, cap, len);
}

int starch_archive_layout(const uint64_t* unit_of, const uint64_t* bytes, uint64_t nseg, uint64_t base,
                          uint64_t* order, uint64_t* offset, uint64_t* end)
{
    if (!end || (nseg && (!unit_of || !bytes || !order || !offset))) return STARCH_ERR_ARG;
    std::vector<uint64_t> o, f;
    shard::layout(unit_of, bytes, nseg, base, o, f, end);
    if (nseg) {
        memcpy(order, o.data(), nseg * sizeof(uint64_t));
        memcpy(offset, f.data(), nseg * sizeof(uint64_t));
    }
    return STARCH_OK;
}

// host only: no context, no GPU
int starch_archive_index(const void* archive, uint64_t n, starch_index_entry* out, uint64_t cap, uint64_t* count,
                         char* names, uint64_t names_cap, uint64_t* names_len, int* compression_method,
                         int* block_size_100k)
{
    if (!archive || !count) return STARCH_ERR_ARG;
    try {
        uint64_t index_off = 0;
        ArchiveInfo info;
        const std::vector<IndexEntry> idx =
            read_index(static_cast<const uint8_t*>(archive), n, &index_off, &info);
        check_bounds(idx, index_off);
        uint64_t nb = 0;
        for (const IndexEntry& e : idx) nb += e.chr.size();
        *count = idx.size();
        if (names_len) *names_len = nb;
        if (compression_method) *compression_method = info.format == "gzip" ? STARCH_METHOD_GZIP : STARCH_METHOD_BZIP2;
        if (block_size_100k) *block_size_100k = info.block_size_100k;
        if (!out && !names) return STARCH_OK;   // sizing call
        if ((out && cap < idx.size()) || (names && names_cap < nb)) return STARCH_ERR_MEM;
        uint64_t no = 0;
        for (size_t k = 0; k < idx.size(); ++k) {
            const IndexEntry& e = idx[k];
            if (out)
                out[k] = starch_index_entry{no, e.chr.size(), e.offset, e.size, e.line_count, e.text_bytes,
                                            e.n_blocks, e.combined_crc, e.has_base_counts ? 1 : 0,
                                            e.base_unique, e.base_nonunique};
            if (names && !e.chr.empty()) memcpy(names + no, e.chr.data(), e.chr.size());
            no += e.chr.size();
        }
        return STARCH_OK;
    } catch (const StarchError& e) {
        return e.code;
    } catch (const std::exception&) {
        return STARCH_ERR_INTERNAL;
    }
}

int starch_archive_note(const void* archive, uint64_t n, char* buf, uint64_t cap, uint64_t* len)
{
    if (!archive || !len) return STARCH_ERR_ARG;
    try {
        uint64_t index_off = 0;
        ArchiveInfo info;
        read_index(static_cast<const uint8_t*>(archive), n, &index_off, &info);
        *len = info.note.size();
        if (!buf) return STARCH_OK;
        if (cap < info.note.size()) return STARCH_ERR_MEM;
        if (!info.note.empty()) memcpy(buf, info.note.data(), info.note.size());
        return STARCH_OK;
    } catch (const StarchError& e) {
        return e.code;
    } catch (const std::exception&) {
        return STARCH_ERR_INTERNAL;
    }
}

}  // extern "C"
