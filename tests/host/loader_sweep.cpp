// loader_sweep.cpp — the host-only readers of files from other programs (gs_hnswio_parse.cpp, gs_bigsi_file.cpp; SPEC.md 16; gs_hmm_parse.cpp; SPEC.md 13) run as a plain C++ program,
// the way a Rust or C++ host calls them: no Python, no HIP runtime, and an address space of 2 GiB, which bounds what a hostile header may allocate.
//
//   loader_sweep <directory>      the directory holds cases.txt and the files it names (tests/loader_case_dir.py writes it):
//     hnswrs <name> <code>                              <name>.hnsw.graph + <name>.hnsw.data must verify to <code>
//     gsbx <name> <code>                                <name>.gsbx must verify to <code>
//     sweep_hnswrs <name> <g|d> <p|f|x> <pos> <code>    the graph or data file of <name> cut to <pos> bytes (p), or with byte <pos> set to 0xFF (f) or ^ 1 (x)
//     sweep_gsbx <name> <p|f|x> <pos> <code>            the same of <name>.gsbx
//     hmm <name> <code>                                 the profile text <name>.hmm must parse (gs_hmm_parse_mem) to <code>
//     sweep_hmm <name> <p|f|x> <pos> <code>             the same of <name>.hmm, parsed from memory
// prints "N files, S surprises"; a surprise is a code other than the listed one, or a C++ exception that reached this program. Exit status 0 iff S = 0.
// Built without the address-space limit (-DLOADER_SWEEP_NO_RLIMIT) for the sanitizer run, whose shadow memory needs terabytes of address space.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <sys/resource.h>
#include <fstream>
#include <iterator>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "../../include/gsearch_amd.h"

namespace gs {
static char g_err[512];
void set_error(const char *fmt, ...)          // the library's own lives in gs_ctx.hip, which this program does not link
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace gs

static std::string slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static bool spit(const std::string &path, const std::string &bytes)
{
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), (std::streamsize)bytes.size());
    return (bool)f.flush();
}
static std::string mutate(const std::string &b, char kind, size_t pos)
{
    if (kind == 'p') return b.substr(0, pos);
    std::string m = b;
    if (pos < m.size()) m[pos] = kind == 'f' ? (char)0xFF : (char)(m[pos] ^ 1);
    return m;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: loader_sweep <directory>\n"); return 2; }
#ifndef LOADER_SWEEP_NO_RLIMIT
    struct rlimit lim = {(rlim_t)2 << 30, (rlim_t)2 << 30};
    if (setrlimit(RLIMIT_AS, &lim) != 0) { perror("setrlimit"); return 2; }
#endif
    const std::string dir = argv[1];
    std::ifstream list(dir + "/cases.txt");
    if (!list) { fprintf(stderr, "cannot read %s/cases.txt\n", dir.c_str()); return 2; }
    std::map<std::string, std::string> cache;
    auto bytes_of = [&](const std::string &path) -> const std::string & { auto it = cache.find(path); return it != cache.end() ? it->second : (cache[path] = slurp(path)); };
    unsigned long files = 0, surprises = 0;
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream in(line);
        std::string what, name, which, kind; size_t pos = 0; int want = 0, got = 1;
        if (!(in >> what >> name)) continue;
        try {
            if (what == "hnswrs" && in >> want) got = gs_hnswrs_verify((dir + "/" + name).c_str(), nullptr);
            else if (what == "gsbx" && in >> want) got = gs_bigsi_verify((dir + "/" + name + ".gsbx").c_str(), nullptr);
            else if (what == "sweep_hnswrs" && in >> which >> kind >> pos >> want) {
                const std::string g = dir + "/" + name + ".hnsw.graph", d = dir + "/" + name + ".hnsw.data";
                if (!spit(dir + "/_sweep.hnsw.graph", which == "g" ? mutate(bytes_of(g), kind[0], pos) : bytes_of(g)) ||
                    !spit(dir + "/_sweep.hnsw.data", which == "d" ? mutate(bytes_of(d), kind[0], pos) : bytes_of(d))) { fprintf(stderr, "cannot write into %s\n", dir.c_str()); return 2; }
                got = gs_hnswrs_verify((dir + "/_sweep").c_str(), nullptr);
            }
            else if (what == "sweep_gsbx" && in >> kind >> pos >> want) {
                if (!spit(dir + "/_sweep.gsbx", mutate(bytes_of(dir + "/" + name + ".gsbx"), kind[0], pos))) { fprintf(stderr, "cannot write into %s\n", dir.c_str()); return 2; }
                got = gs_bigsi_verify((dir + "/_sweep.gsbx").c_str(), nullptr);
            }
            else if (what == "hmm" && in >> want) { const std::string &t = bytes_of(dir + "/" + name + ".hmm"); got = gs_hmm_parse_mem(t.data(), t.size(), 0, nullptr, nullptr, 0, nullptr); }
            else if (what == "sweep_hmm" && in >> kind >> pos >> want) {
                const std::string t = mutate(bytes_of(dir + "/" + name + ".hmm"), kind[0], pos);
                got = gs_hmm_parse_mem(t.data(), t.size(), 0, nullptr, nullptr, 0, nullptr);
            }
            else { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
            files++;
            if (got != want) { surprises++; printf("SURPRISE %s: code %d, listed %d (%s)\n", line.c_str(), got, want, got ? gs::g_err : "accepted"); }
        }
        catch (const std::exception &e) { files++; surprises++; printf("SURPRISE %s: exception %s\n", line.c_str(), e.what()); }
        catch (...) { files++; surprises++; printf("SURPRISE %s: exception\n", line.c_str()); }
    }
    printf("%lu files, %lu surprises\n", files, surprises);
    return surprises ? 1 : 0;
}
