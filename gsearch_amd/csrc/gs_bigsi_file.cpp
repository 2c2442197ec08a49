// gs_bigsi_file.cpp — reading a .gsbx file on the host (layout: above gs_bigsi_save in gs_bigsi.hip; order of the checks and their codes: SPEC.md 16.2).
// The file is untrusted: n_colours and bloom_size are compared with the size of the file before anything is allocated from them - on the host or, by
// gs_bigsi_load, on the device -, every allocation sits inside a try, and no exception leaves this unit.
#include <errno.h>
#include <string.h>
#include <sys/stat.h>
#include <algorithm>
#include <exception>
#include "gs_bigsi_file.hpp"

namespace gs {
namespace {

int read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n ? 0 : -1; }
struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } };

// SPEC 16.2 steps 1-2: the fixed header as it stands in the file, nothing judged but magic and version. *end = the offset behind it.
int read_header(FILE *f, const char *path, gs_bigsi_file_description *d, uint64_t *end)
{
    char magic[8]; uint32_t head[5] = {0, 0, 0, 0, 0}; uint64_t B = 0, n = 0;
    int bad = read_all(f, magic, 8) | read_all(f, head, 16);
    const bool mini = !bad && head[0] == BX_VERSION_MINI;
    if (mini) bad |= read_all(f, head + 4, 4);
    bad |= read_all(f, &B, 8) | read_all(f, &n, 8);
    GS_REQUIRE(!bad && memcmp(magic, BX_MAGIC, 8) == 0 && (head[0] == BX_VERSION || mini), GS_ERR_IO, "%s is not a bigsig index of this library (versions %u and %u)", path,
               BX_VERSION, BX_VERSION_MINI);
    memset(d, 0, sizeof *d);
    d->version = head[0]; d->k = head[1]; d->num_hash = head[2]; d->data_t = head[3]; d->minimizer_len = head[4];
    d->bloom_size = B; d->n_colours = n; d->row_words = n / 64 + (n % 64 != 0);
    *end = mini ? 44 : 40;
    return GS_OK;
}

int parse_body(const char *path, BigsiFile *o, FILE **keep)
{
    FILE *f = fopen(path, "rb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot read %s: %s", path, strerror(errno));
    Closer closer{f};
    uint64_t at = 0;
    int rc = read_header(f, path, &o->desc, &at);
    if (rc) return rc;
    gs_bigsi_file_description &d = o->desc;
    const uint64_t n = d.n_colours, B = d.bloom_size, wu = d.row_words;
    GS_REQUIRE((d.version != BX_VERSION_MINI || (d.minimizer_len >= 1 && d.minimizer_len < d.k)) && n < ((uint64_t)1 << 32), GS_ERR_IO,
               "%s is not a bigsig index of this library (minimizer length %u, k %u, %llu colours)", path, d.minimizer_len, d.k, (unsigned long long)n);
    // the file against its header, BEFORE anything is sized from it: with empty accessions it holds 4 + 16 bytes per colour and the matrix
    struct stat st;
    GS_REQUIRE(fstat(fileno(f), &st) == 0 && st.st_size >= 0, GS_ERR_IO, "cannot stat %s", path);
    const unsigned __int128 size = (uint64_t)st.st_size, matrix = (unsigned __int128)B * wu * 8;
    GS_REQUIRE(size >= at + (unsigned __int128)n * 20 + matrix, GS_ERR_IO, "%s is cut short: %llu bytes cannot hold %llu colours and %llu rows", path,
               (unsigned long long)st.st_size, (unsigned long long)n, (unsigned long long)B);
    o->names.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t l = 0;
        GS_REQUIRE(read_all(f, &l, 4) == 0 && l <= (1u << 20), GS_ERR_IO, "%s is cut short (accession %llu)", path, (unsigned long long)i);
        at += 4 + (uint64_t)l;
        GS_REQUIRE(size >= at, GS_ERR_IO, "%s is cut short (accession %llu)", path, (unsigned long long)i);
        o->names[i].resize(l);
        GS_REQUIRE(read_all(f, &o->names[i][0], l) == 0, GS_ERR_IO, "%s is cut short (accession %llu)", path, (unsigned long long)i);
        if (l) d.has_accessions = 1;
    }
    GS_REQUIRE(size == at + (unsigned __int128)n * 16 + matrix, GS_ERR_IO, "%s: size %llu does not match its header (%llu colours, %llu rows): cut short or bytes after the last row", path,
               (unsigned long long)st.st_size, (unsigned long long)n, (unsigned long long)B);
    o->t.resize(n); o->q.resize(n);
    GS_REQUIRE((read_all(f, o->t.data(), 8 * n) | read_all(f, o->q.data(), 8 * n)) == 0, GS_ERR_IO, "%s is cut short", path);
    o->rows_at = at + n * 16;
    // only now the parameters (GS_ERR_INVALID: the file is whole, what it describes is not an index of this library)
    memset(&o->prm, 0, sizeof o->prm);
    o->prm.k = d.k; o->prm.num_hash = d.num_hash; o->prm.data_t = d.data_t; o->prm.bloom_size = B;
    if ((rc = gs_bigsi_check_params(&o->prm))) return rc;
    if (keep) { *keep = f; closer.f = nullptr; }
    return GS_OK;
}

}  // namespace

int bigsi_file_parse(const char *path, BigsiFile *out, FILE **keep)
{
    try { return parse_body(path, out, keep); }
    catch (const std::exception &e) { set_error("%s: not enough host memory for what its header names (%s)", path, e.what()); return GS_ERR_IO; }
    catch (...) { set_error("%s: reading the index failed", path); return GS_ERR_IO; }
}

}  // namespace gs

extern "C" {

int gs_bigsi_check_params(const gs_bigsi_params *p)
{
    GS_REQUIRE(p, GS_ERR_INVALID, "null parameters");
    GS_REQUIRE(p->k >= 1 && p->k <= GS_BIGSI_KMAX, GS_ERR_INVALID, "bigsig: k = %u outside 1..32", p->k);
    GS_REQUIRE(p->num_hash >= 1 && p->num_hash <= GS_BIGSI_HMAX, GS_ERR_INVALID, "bigsig: num_hash = %u outside 1..16", p->num_hash);
    GS_REQUIRE(p->bloom_size >= 1 && p->bloom_size < GS_BIGSI_BMAX, GS_ERR_INVALID, "bigsig: bloom_size = %llu outside 1..2^40-1", (unsigned long long)p->bloom_size);
    GS_REQUIRE(p->data_t == GS_DATA_DNA || p->data_t == GS_DATA_DNA_FWD, GS_ERR_INVALID, "bigsig: data type %u is not DNA", p->data_t);
    GS_REQUIRE(p->minimizer == 0, GS_ERR_UNSUPPORTED, "bigsig: the minimizer mode (-m) is not implemented");
    GS_REQUIRE(p->coverage_filter == 0, GS_ERR_UNSUPPORTED, "bigsig: the coverage filter (-f) is not implemented");
    return GS_OK;
}

/* the fixed header of a .gsbx file as it stands in the file, nothing judged but magic and version */
int gs_bigsi_describe(const char *path, gs_bigsi_file_description *out)
{
    GS_REQUIRE(path && out, GS_ERR_INVALID, "null argument");
    FILE *f = fopen(path, "rb");
    GS_REQUIRE(f, GS_ERR_IO, "cannot read %s: %s", path, strerror(errno));
    gs::Closer closer{f};
    uint64_t end = 0;
    return gs::read_header(f, path, out, &end);
}

/* everything gs_bigsi_load checks before it asks the device for memory, with its codes and messages; no context. out (optional): the header, whether any
 * accession is non-empty, and the digest of everything behind the header (SPEC 16.3) */
int gs_bigsi_verify(const char *path, gs_bigsi_file_description *out)
{
    GS_REQUIRE(path, GS_ERR_INVALID, "null argument");
    try {
        gs::BigsiFile bf; FILE *f = nullptr;
        const int rc = gs::bigsi_file_parse(path, &bf, &f);
        if (rc) return rc;
        gs::Closer closer{f};
        uint64_t h = gs::FNV_BASIS;
        for (const std::string &s : bf.names) { const uint32_t l = (uint32_t)s.size(); h = gs::fnv1a(h, &l, 4); h = gs::fnv1a(h, s.data(), l); }
        h = gs::fnv1a(h, bf.t.data(), 8 * bf.t.size()); h = gs::fnv1a(h, bf.q.data(), 8 * bf.q.size());
        std::vector<uint8_t> buf((size_t)1 << 20);
        for (size_t got; (got = fread(buf.data(), 1, buf.size(), f)) > 0;) h = gs::fnv1a(h, buf.data(), got);
        bf.desc.digest = h;
        if (out) *out = bf.desc;
        return GS_OK;
    }
    catch (...) { gs::set_error("%s: verifying the index failed", path); return GS_ERR_IO; }
}

}  // extern "C"
