// gs_hnswio_parse.cpp — reading an hnsw_rs dump on the host: the byte layout is the one in the header of gs_hnswio.hip (restated AS RECALLED, see
// there), the order of the checks and their codes are SPEC.md 16.1. Both files come from another program and are untrusted: every size they name is
// compared with the sizes of the files before anything is allocated from it, every allocation sits inside a try, and no exception leaves this unit.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <algorithm>
#include <exception>
#include <string>
#include <unordered_map>
#include "gs_hnswio_parse.hpp"

namespace gs {
namespace {

using namespace fmt;
constexpr uint32_t NB_LAYER = NB_LAYER_MAX;
constexpr uint64_t POINT_MIN = 4 + 8 + 1 + 4 + NB_LAYER, LAYER_HDR = 4 + 8, ENTRY = 8 + 1 + 4;      // a point without neighbours; a layer header; the entry point

struct Rd {
    FILE *f; bool ok = true;
    template <class T> T get() { T v{}; ok = ok && fread(&v, sizeof(T), 1, f) == 1; return v; }
    void bytes(void *p, size_t n) { ok = ok && (n == 0 || fread(p, 1, n, f) == n); }
    std::string str() { const uint64_t n = get<uint64_t>(); if (!ok || n > 4096) { ok = false; return std::string(); } std::string s(n, '\0'); bytes(&s[0], n); return s; }
};
struct Closer { FILE *a, *b; ~Closer() { if (a) fclose(a); if (b) fclose(b); } };

int kind_of_tname(const std::string &t) { return t == "f32" ? GS_KIND_F32 : t == "u32" ? GS_KIND_U32 : t == "u64" ? GS_KIND_U64 : t == "u16" ? GS_KIND_U16 : -1; }
size_t esz_of(int kind) { return kind == GS_KIND_U16 ? 2 : (kind == GS_KIND_U64 ? 8 : 4); }
bool file_size(FILE *f, uint64_t *out) { struct stat st; if (fstat(fileno(f), &st) != 0 || st.st_size < 0) return false; *out = (uint64_t)st.st_size; return true; }

// SPEC 16.1 steps 2-3: the description as it stands in the file, nothing judged but its magic. *end = the offset behind it.
int read_description(Rd &g, const char *gname, gs_hnswrs_description *d, std::string *distname, std::string *tname, uint64_t *end)
{
    const uint32_t magic = g.get<uint32_t>();
    GS_REQUIRE(g.ok, GS_ERR_IO, "truncated description in %s", gname);
    GS_REQUIRE(magic != MAGICDESCR_2, GS_ERR_UNSUPPORTED, "%s is a format-2 dump (bincode vectors); re-dump it with hnsw_rs >= 0.2", gname);
    GS_REQUIRE(magic == MAGICDESCR_3, GS_ERR_IO, "%s is not an hnsw_rs graph dump (magic %08x)", gname, magic);
    memset(d, 0, sizeof *d);
    d->dump_mode = g.get<uint8_t>(); d->max_nb_conn = g.get<uint8_t>(); d->nb_layer = g.get<uint8_t>();
    d->ef = g.get<uint64_t>(); d->nb_point = g.get<uint64_t>(); d->dimension = g.get<uint64_t>();
    *distname = g.str(); *tname = g.str();
    GS_REQUIRE(g.ok, GS_ERR_IO, "truncated description in %s", gname);
    d->kind = kind_of_tname(*tname);
    memcpy(d->distance, distname->data(), std::min(distname->size(), sizeof(d->distance) - 1));
    memcpy(d->t_name, tname->data(), std::min(tname->size(), sizeof(d->t_name) - 1));
    *end = (uint64_t)ftell(g.f);
    return GS_OK;
}

int parse_body(const char *basename, HnswrsDump *o)
{
    const std::string gname = std::string(basename) + ".hnsw.graph", dname = std::string(basename) + ".hnsw.data";
    FILE *fg = fopen(gname.c_str(), "rb"), *fd = fopen(dname.c_str(), "rb");
    Closer closer{fg, fd};
    GS_REQUIRE(fg && fd, GS_ERR_IO, "cannot open %s / %s", gname.c_str(), dname.c_str());
    Rd g{fg}, d{fd};
    std::string distname, tname;
    uint64_t desc_end = 0, gsize = 0, dsize = 0;
    int rc = read_description(g, gname.c_str(), &o->desc, &distname, &tname, &desc_end);
    if (rc) return rc;
    const gs_hnswrs_description &ds = o->desc;
    GS_REQUIRE(ds.dump_mode == 1, GS_ERR_UNSUPPORTED, "light dumps (graph without data) cannot be searched");
    GS_REQUIRE(ds.nb_layer == NB_LAYER, GS_ERR_IO, "description says %u layers, hnsw_rs always dumps 16", ds.nb_layer);
    GS_REQUIRE(distname.find("DistHamming") != std::string::npos, GS_ERR_UNSUPPORTED, "distance %s: gsearch databases use DistHamming", ds.distance);
    GS_REQUIRE(ds.kind >= 0, GS_ERR_UNSUPPORTED, "element type %s is not a signature type of gsearch", ds.t_name);
    const uint64_t n = ds.nb_point, dim = ds.dimension;
    GS_REQUIRE(ds.max_nb_conn >= 2 && n >= 1 && n < ((uint64_t)1 << 31) && dim >= 1 && dim < ((uint64_t)1 << 31) && ds.ef <= 0xFFFFFFFFull, GS_ERR_IO,
               "implausible description (M %u, n %llu, dim %llu, ef %llu)", ds.max_nb_conn, (unsigned long long)n, (unsigned long long)dim, (unsigned long long)ds.ef);
    const uint32_t M = ds.max_nb_conn, ML = NB_LAYER, m = (uint32_t)dim;
    const size_t esz = esz_of(ds.kind), row = esz * m;
    // the sizes of the two files against the description, BEFORE anything is sized from it
    GS_REQUIRE(file_size(fg, &gsize) && file_size(fd, &dsize), GS_ERR_IO, "cannot stat %s / %s", gname.c_str(), dname.c_str());
    const unsigned __int128 dwant = (unsigned __int128)12 + (unsigned __int128)n * (20 + (uint64_t)row);
    GS_REQUIRE(dwant == (unsigned __int128)dsize, GS_ERR_IO, "%s: size %llu does not match the description (%llu vectors of %llu bytes)", dname.c_str(),
               (unsigned long long)dsize, (unsigned long long)n, (unsigned long long)row);
    const uint64_t gmin = desc_end + 1 + ML * LAYER_HDR + n * POINT_MIN + ENTRY;      // n < 2^31: no overflow
    GS_REQUIRE(gsize >= gmin, GS_ERR_IO, "%s: size %llu is too short for %llu points", gname.c_str(), (unsigned long long)gsize, (unsigned long long)n);
    o->kind = ds.kind; o->M = M; o->m = m; o->n = n;
    o->sigs.resize((size_t)n * row); o->oid.resize(n);
    // data file. DataIds: gsearch's are the dictionary ranks 0..n-1 (dnasketch.rs:429-433) and then ARE the node numbers of this library; any other set of
    // distinct ids is kept as the caller's ids (gs_index_set_ids) over nodes numbered in the order of the data file
    GS_REQUIRE(d.get<uint32_t>() == MAGICDATAP && d.get<uint64_t>() == dim && d.ok, GS_ERR_IO, "%s: bad header", dname.c_str());
    bool dense = true;
    {
        std::vector<uint8_t> have(n, 0);
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t mg = d.get<uint32_t>(); const uint64_t id = d.get<uint64_t>(), nb = d.get<uint64_t>();
            GS_REQUIRE(d.ok && mg == MAGICDATAP && nb == row, GS_ERR_IO, "%s: bad vector record %llu", dname.c_str(), (unsigned long long)i);
            o->oid[i] = id;
            if (id >= n || have[id]) dense = false; else have[id] = 1;
            GS_REQUIRE(fseek(fd, (long)row, SEEK_CUR) == 0, GS_ERR_IO, "%s is truncated", dname.c_str());
        }
    }
    o->dense = dense;
    std::unordered_map<uint64_t, uint64_t> node_of;
    if (!dense) {
        node_of.reserve(n * 2);
        for (uint64_t i = 0; i < n; i++) GS_REQUIRE(node_of.emplace(o->oid[i], i).second, GS_ERR_IO, "%s: id %llu appears twice", dname.c_str(), (unsigned long long)o->oid[i]);
    }
    auto node = [&](uint64_t id, bool *ok) -> uint64_t {          // DataId -> node number
        if (dense) { if (id >= n) { *ok = false; return 0; } return id; }
        auto it = node_of.find(id);
        if (it == node_of.end()) { *ok = false; return 0; }
        return it->second;
    };
    GS_REQUIRE(fseek(fd, 12, SEEK_SET) == 0, GS_ERR_IO, "%s: seek", dname.c_str());
    for (uint64_t i = 0; i < n; i++) {
        (void)d.get<uint32_t>(); const uint64_t id = d.get<uint64_t>(); (void)d.get<uint64_t>();
        bool ok = true;
        d.bytes(o->sigs.data() + node(id, &ok) * row, row);
        GS_REQUIRE(d.ok && ok, GS_ERR_IO, "%s is truncated", dname.c_str());
    }
    // graph
    GS_REQUIRE(g.get<uint8_t>() == NB_LAYER && g.ok, GS_ERR_IO, "%s: bad layer count", gname.c_str());
    o->lv.assign(n, 0xFF); o->d0.assign(n, 0); o->n0.assign((size_t)n * 2 * M, 0); o->c0.assign((size_t)n * 2 * M, 0); o->up.assign(n, -1);
    struct UpperList { uint32_t u, l, cnt; uint64_t at; };         // list l of upper node u: cnt keys (count << 32 | id) from ukeys[at]
    std::vector<UpperList> ulists; std::vector<uint64_t> ukeys;
    uint64_t seen = 0, U = 0, keys[255];
    const float fm = (float)m;
    for (uint32_t L = 0; L < ML; L++) {
        GS_REQUIRE(g.get<uint32_t>() == MAGICLAYER && g.ok, GS_ERR_IO, "%s: layer %u header missing", gname.c_str(), L);
        const uint64_t np = g.get<uint64_t>();
        GS_REQUIRE(g.ok && np <= n - seen, GS_ERR_IO, "%s: layer %u claims %llu points", gname.c_str(), L, (unsigned long long)np);
        for (uint64_t j = 0; j < np; j++) {
            bool idok = true;
            const uint32_t mg = g.get<uint32_t>(); const uint64_t id = node(g.get<uint64_t>(), &idok); const uint8_t pl = g.get<uint8_t>(); (void)g.get<int32_t>();
            GS_REQUIRE(g.ok && idok && mg == MAGICPOINT && id < n && pl == L && o->lv[id] == 0xFF, GS_ERR_IO, "%s: bad point record (layer %u, rank %llu)", gname.c_str(), L, (unsigned long long)j);
            o->lv[id] = (uint8_t)L;
            if (L > 0) o->up[id] = (int32_t)U++;
            for (uint32_t l = 0; l < ML; l++) {
                const uint8_t cnt = g.get<uint8_t>();
                for (uint32_t t = 0; t < cnt; t++) {
                    bool nok = true;
                    const uint64_t nid = node(g.get<uint64_t>(), &nok); (void)g.get<uint8_t>(); (void)g.get<int32_t>(); const float dist = g.get<float>();
                    GS_REQUIRE(g.ok && nok && nid < n && dist >= 0.0f && dist <= 1.0f, GS_ERR_IO, "%s: bad neighbour of point %llu", gname.c_str(), (unsigned long long)id);
                    keys[t] = ((uint64_t)(uint32_t)llrintf(dist * fm) << 32) | nid;
                }
                GS_REQUIRE(g.ok, GS_ERR_IO, "%s is truncated", gname.c_str());
                GS_REQUIRE(cnt == 0 || l <= L, GS_ERR_IO, "%s: point %llu of layer %u has neighbours at layer %u", gname.c_str(), (unsigned long long)id, L, l);
                std::sort(keys, keys + cnt);                          // this library keeps lists in (count, id) order
                if (l == 0) {
                    GS_REQUIRE(cnt <= 2 * M, GS_ERR_IO, "%s: point %llu has %u layer-0 neighbours, more than 2M", gname.c_str(), (unsigned long long)id, cnt);
                    o->d0[id] = cnt;
                    for (uint32_t t = 0; t < cnt; t++) { o->n0[(uint64_t)id * 2 * M + t] = (uint32_t)keys[t]; o->c0[(uint64_t)id * 2 * M + t] = (uint32_t)(keys[t] >> 32); }
                } else if (cnt) {
                    GS_REQUIRE(cnt <= M, GS_ERR_IO, "%s: point %llu has %u neighbours at layer %u, more than M", gname.c_str(), (unsigned long long)id, cnt, l);
                    ulists.push_back(UpperList{(uint32_t)o->up[id], l, cnt, (uint64_t)ukeys.size()});
                    ukeys.insert(ukeys.end(), keys, keys + cnt);
                }
            }
        }
        seen += np;
    }
    GS_REQUIRE(seen == n, GS_ERR_IO, "%s holds %llu points, its description says %llu", gname.c_str(), (unsigned long long)seen, (unsigned long long)n);
    bool eok = true;
    const uint64_t entry = node(g.get<uint64_t>(), &eok); (void)g.get<uint8_t>(); (void)g.get<int32_t>();
    GS_REQUIRE(g.ok && eok && entry < n, GS_ERR_IO, "%s: entry point missing", gname.c_str());
    GS_REQUIRE((uint64_t)ftell(fg) == gsize, GS_ERR_IO, "%s: bytes after the entry point", gname.c_str());
    o->U = U; o->entry = entry;
    const uint64_t Ua = std::max<uint64_t>(U, 1);
    o->dU.assign(Ua * ML, 0); o->nU.assign(Ua * ML * M, 0); o->cU.assign(Ua * ML * M, 0);
    for (const UpperList &e : ulists) {
        const uint64_t at = (uint64_t)e.u * ML + (e.l - 1);
        o->dU[at] = e.cnt;
        for (uint32_t t = 0; t < e.cnt; t++) { o->nU[at * M + t] = (uint32_t)ukeys[e.at + t]; o->cU[at * M + t] = (uint32_t)(ukeys[e.at + t] >> 32); }
    }
    // what gs_index_import asks of a graph, here so that a refusal needs no device (GS_ERR_INVALID: the files are well formed, the graph is not)
    if ((rc = graph_validate(n, M, ML, o->lv.data(), (int64_t)entry, o->d0.data(), o->n0.data(), o->up.data(), U, o->dU.data(), o->nU.data()))) return rc;
    o->desc.n_upper = U; o->desc.entry = entry; o->desc.ids_are_nodes = dense ? 1 : 0;
    return GS_OK;
}

// SPEC 16.3: per node in node order its id, level, vector and the lists of layers 0..level as (degree, then neighbour and count of every entry), then the entry point
uint64_t dump_digest(const HnswrsDump &o)
{
    uint64_t h = FNV_BASIS;
    const size_t row = esz_of(o.kind) * o.m;
    const uint32_t M = o.M, ML = NB_LAYER;
    for (uint64_t i = 0; i < o.n; i++) {
        const uint64_t id = o.dense ? i : o.oid[i];
        h = fnv1a(h, &id, 8); h = fnv1a(h, &o.lv[i], 1); h = fnv1a(h, o.sigs.data() + i * row, row);
        for (uint32_t l = 0; l <= o.lv[i]; l++) {
            const uint64_t at = l ? (uint64_t)o.up[i] * ML + (l - 1) : 0;
            const uint32_t deg = l ? o.dU[at] : o.d0[i];
            const uint32_t *nb = l ? &o.nU[at * M] : &o.n0[i * 2 * M], *cn = l ? &o.cU[at * M] : &o.c0[i * 2 * M];
            h = fnv1a(h, &deg, 4);
            for (uint32_t t = 0; t < deg; t++) { h = fnv1a(h, &nb[t], 4); h = fnv1a(h, &cn[t], 4); }
        }
    }
    return fnv1a(h, &o.entry, 8);
}

}  // namespace

int hnswrs_parse(const char *basename, HnswrsDump *out)
{
    try { return parse_body(basename, out); }
    catch (const std::exception &e) { set_error("%s: not enough host memory for what its description names (%s)", basename, e.what()); return GS_ERR_IO; }
    catch (...) { set_error("%s: reading the dump failed", basename); return GS_ERR_IO; }
}

int graph_validate(uint64_t n, uint32_t M, uint32_t ML, const uint8_t *levels, int64_t entry, const uint32_t *deg0, const uint32_t *nbr0,
                   const int32_t *upidx, uint64_t n_upper, const uint32_t *degU, const uint32_t *nbrU)
{
    std::vector<uint8_t> taken;
    try { taken.assign(n_upper, 0); }
    catch (const std::exception &) { set_error("not enough host memory to check %llu upper nodes", (unsigned long long)n_upper); return GS_ERR_IO; }
    int top = 0;
    for (uint64_t i = 0; i < n; i++) {
        GS_REQUIRE(levels[i] < ML, GS_ERR_INVALID, "level of node %llu out of range", (unsigned long long)i);
        GS_REQUIRE(deg0[i] <= 2 * M, GS_ERR_INVALID, "degree of node %llu out of range", (unsigned long long)i);
        for (uint32_t t = 0; t < deg0[i]; t++) GS_REQUIRE(nbr0[i * 2 * M + t] < n, GS_ERR_INVALID, "neighbour id out of range");
        GS_REQUIRE((levels[i] > 0) == (upidx[i] >= 0), GS_ERR_INVALID, "upidx inconsistent with level at node %llu", (unsigned long long)i);
        if (upidx[i] >= 0) {
            GS_REQUIRE((uint64_t)upidx[i] < n_upper, GS_ERR_INVALID, "upidx of node %llu out of range", (unsigned long long)i);
            GS_REQUIRE(!taken[upidx[i]], GS_ERR_INVALID, "upidx %d of node %llu belongs to another node already", upidx[i], (unsigned long long)i);
            taken[upidx[i]] = 1;
            for (uint32_t l = 1; l <= levels[i]; l++) {
                const uint64_t o = (uint64_t)upidx[i] * ML + (l - 1);
                GS_REQUIRE(degU[o] <= M, GS_ERR_INVALID, "degree of node %llu at layer %u out of range", (unsigned long long)i, l);
                for (uint32_t t = 0; t < degU[o]; t++) {
                    const uint32_t e = nbrU[o * M + t];
                    GS_REQUIRE(e < n && levels[e] < ML && levels[e] >= l, GS_ERR_INVALID, "node %llu links to %u at layer %u, which does not reach that layer", (unsigned long long)i, e, l);
                }
            }
        }
        if (levels[i] > top) top = levels[i];
    }
    GS_REQUIRE(levels[entry] == top, GS_ERR_INVALID, "entry point is not on the top layer");
    return GS_OK;
}

}  // namespace gs

extern "C" {

/* get_hnsw_type (reloadhnsw.rs:13-38): the description of <basename>.hnsw.graph as it stands in the file, nothing judged but its magic and that it is whole */
int gs_hnswrs_describe(const char *basename, gs_hnswrs_description *out)
{
    GS_REQUIRE(basename && out, GS_ERR_INVALID, "null argument");
    try {
        const std::string gname = std::string(basename) + ".hnsw.graph";
        FILE *fg = fopen(gname.c_str(), "rb");
        GS_REQUIRE(fg, GS_ERR_IO, "cannot open %s", gname.c_str());
        gs::Closer closer{fg, nullptr};
        gs::Rd g{fg};
        std::string distname, tname; uint64_t end = 0;
        return gs::read_description(g, gname.c_str(), out, &distname, &tname, &end);
    }
    catch (...) { gs::set_error("%s: reading the description failed", basename); return GS_ERR_IO; }
}

/* everything gs_index_load_hnswrs checks before the device, with its codes and messages; no context. out (optional): the description, and what the
 * load would build: n_upper, entry, ids_are_nodes, digest (SPEC 16.3) */
int gs_hnswrs_verify(const char *basename, gs_hnswrs_description *out)
{
    GS_REQUIRE(basename, GS_ERR_INVALID, "null argument");
    try {
        gs::HnswrsDump dump;
        const int rc = gs::hnswrs_parse(basename, &dump);
        if (rc) return rc;
        dump.desc.digest = gs::dump_digest(dump);
        if (out) *out = dump.desc;
        return GS_OK;
    }
    catch (...) { gs::set_error("%s: verifying the dump failed", basename); return GS_ERR_IO; }
}

}  // extern "C"
