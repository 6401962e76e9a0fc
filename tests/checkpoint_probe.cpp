// Stand-alone probe of artspeech_amd/csrc/checkpoint.h for tests/test_checkpoint_cpu.py (compiled there with g++, plain and under
// AddressSanitizer + UBSan).  It computes nothing of its own: it hands files to the header's functions and writes down what they return.
//
//   checkpoint_probe reject  FILE                       FILE = records { u64 length | bytes }: one line per record, read_blob's answer
//   checkpoint_probe OP      BLOB OUT [arguments]       BLOB -> read_blob [-> fold [-> OP]]; the resulting tensors go to OUT as
//                                                       { u32 name_len | name | u32 ndim | i32 dims | u64 numel | fp32 data }
// Every blob is copied into a heap buffer of exactly its length before the reader sees it, so a read past the end is a finding of
// the sanitizer.  The first line printed is "ok" or "fail <what the header reported>"; further lines are integers the call returned.
#include "checkpoint.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

namespace ck = checkpoint;

static std::vector<unsigned char> file_bytes(const char* path)
{
    std::vector<unsigned char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    unsigned char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

// read_blob on a heap copy of exactly n bytes
static bool read_exact(const unsigned char* p, size_t n, ck::Map* out)
{
    std::unique_ptr<unsigned char[]> heap(new unsigned char[n]);
    if (n) std::memcpy(heap.get(), p, n);
    return ck::read_blob(heap.get(), n, out);
}

static void dump(FILE* f, const std::string& name, const std::vector<int>& dims, const std::vector<float>& v)
{
    const uint32_t nl = (uint32_t)name.size(), nd = (uint32_t)dims.size();
    const uint64_t n = v.size();
    std::fwrite(&nl, 4, 1, f);
    std::fwrite(name.data(), 1, nl, f);
    std::fwrite(&nd, 4, 1, f);
    for (int d : dims) { const int32_t x = d; std::fwrite(&x, 4, 1, f); }
    std::fwrite(&n, 8, 1, f);
    if (n) std::fwrite(v.data(), 4, n, f);
}
static void dump(FILE* f, const ck::Map& m)
{
    for (const auto& kv : m) dump(f, kv.first, kv.second.dims, kv.second.v);
}
static void dump(FILE* f, const ck::Mat& a)
{
    dump(f, "w", {a.G, a.M, a.K, a.T}, a.w);
    dump(f, "w2", {a.G, a.M, a.K2}, a.w2);
    dump(f, "b", {(int)a.b.size()}, a.b);
}

static std::vector<std::string> split(const std::string& s, char sep)
{
    std::vector<std::string> v(1);
    for (char c : s) {
        if (c == sep) v.emplace_back();
        else v.back() += c;
    }
    return v;
}

static int answer(bool ok, const std::string& what = std::string())
{
    if (ok) std::printf("ok\n");
    else std::printf("fail %s\n", what.c_str());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const std::string op = argv[1];
    const std::vector<unsigned char> in = file_bytes(argv[2]);
    if (op == "reject") {
        for (size_t o = 0; o < in.size();) {
            uint64_t n;
            std::memcpy(&n, in.data() + o, 8);
            o += 8;
            ck::Map m;
            std::printf("%d\n", read_exact(in.data() + o, (size_t)n, &m) ? 1 : 0);
            o += n;
        }
        return 0;
    }
    if (argc < 4) return 2;
    const std::vector<std::string> arg(argv + 4, argv + argc);
    struct Out {
        FILE* f;
        ~Out() { if (f) std::fclose(f); }
    } out{std::fopen(argv[3], "wb")};
    if (!out.f) return 2;
    ck::Map raw, m;
    if (!read_exact(in.data(), in.size(), &raw)) return answer(false, "read_blob");
    if (op == "read") { dump(out.f, raw); return answer(true); }
    if (!ck::fold(raw, &m)) return answer(false, "fold");
    if (op == "fold") { dump(out.f, m); return answer(true); }
    if (op == "towers" && arg.size() == 3) {
        if (!ck::merge_twin_towers(&m, arg[0], arg[1], arg[2])) return answer(false, "merge_twin_towers");
        dump(out.f, m);
        return answer(true);
    }
    if (op == "linears" && arg.size() == 3) {
        if (!ck::merge_twin_linears(&m, arg[0], arg[1], arg[2])) return answer(false, "merge_twin_linears");
        dump(out.f, m);
        return answer(true);
    }
    std::string missing;
    ck::Mat a;
    if (op == "concat" && arg.size() >= 2) {                        // same_dims (0 / 1), names
        std::vector<float> v;
        const ck::HostT* first;
        if (!ck::concat(m, {arg.begin() + 1, arg.end()}, arg[0] == "1", &v, &first, &missing)) return answer(false, missing);
        dump(out.f, "v", {(int)v.size()}, v);
        return answer(true);
    }
    if (op == "conv_stack") {
        if (!ck::conv_stack(m, arg, &a, &missing)) return answer(false, missing);
    } else if (op == "conv_fold" && arg.size() == 2) {              // names and shortcut names, each list joined by commas
        if (!ck::conv_fold(m, split(arg[0], ','), split(arg[1], ','), &a, &missing)) return answer(false, missing);
    } else if (op == "qkv") {
        if (!ck::qkv(m, arg, &a, &missing)) return answer(false, missing);
    } else if (op == "lstm_wih") {
        if (!ck::lstm_wih(m, arg, &a, &missing)) return answer(false, missing);
    } else if (op == "lstm_whh_t" && arg.size() == 1) {
        std::vector<float> t;
        int H = 0;
        if (!ck::lstm_whh_t(m, arg[0], &t, &H, &missing)) return answer(false, missing);
        dump(out.f, "t", {2, H, 4 * H}, t);
        return answer(true);
    } else if (op == "fc_all" && arg.size() >= 1) {                 // K, then name:off:S per layer
        std::vector<ck::NormSpec> norms;
        for (size_t i = 1; i < arg.size(); ++i) {
            const std::vector<std::string> p = split(arg[i], ':');
            if (p.size() != 3) return 2;
            norms.push_back({p[0], std::atoi(p[1].c_str()), std::atoi(p[2].c_str())});
        }
        std::unordered_map<std::string, int> row0;
        if (!ck::fc_all(m, norms, std::atoi(arg[0].c_str()), &a, &row0, &missing)) return answer(false, missing);
        answer(true);
        for (const auto& n : norms) std::printf("%s %d\n", n.name.c_str(), row0.at(n.name));
        dump(out.f, a);
        return 0;
    } else if (op == "fne") {
        if (!ck::fne(m, &a, &missing)) return answer(false, missing);
    } else if (op == "direct_image" && arg.size() == 2) {           // a tensor [Cout][1][T], Kp
        const auto it = m.find(arg[0]);
        if (it == m.end()) return answer(false, arg[0]);
        const int Cout = it->second.dim(0), T = (int)(it->second.numel() / Cout), Kp = std::atoi(arg[1].c_str());
        dump(out.f, "w32", {T, Kp, Cout}, ck::direct_image(it->second.v.data(), Cout, T, Kp));
        return answer(true);
    } else if (op == "generator_ok" && arg.size() >= 6) {           // num_mels c0 n_stages n_stacks n_dilations max_taps, ups k's, resblock k's
        std::vector<int32_t> v;
        for (const std::string& s : arg) v.push_back(std::atoi(s.c_str()));
        if (v[2] < 0 || v[3] < 0 || v.size() != (size_t)6 + v[2] + v[3]) return 2;
        const ck::GeneratorShape g = {v[0], v[1], v[2], v[3], v[4], v.data() + 6, v.data() + 6 + v[2], v[5]};
        std::string why;
        return answer(ck::checkpoint_ok(m, g, &why), why);
    } else if (op == "upsample" && arg.size() == 2) {               // "ups.i", u
        const auto wt = m.find(arg[0] + ".weight"), b = m.find(arg[0] + ".bias");
        if (wt == m.end() || b == m.end()) return answer(false, arg[0]);
        const int u = std::atoi(arg[1].c_str()), cin = wt->second.dim(0), cout = wt->second.dim(1);
        if (wt->second.dim(2) != 2 * u) return 2;
        std::unique_ptr<float[]> wc(new float[(size_t)u * cout * cin * 3]);      // (exactly the room the fold may write)
        if (!ck::fold_upsample(wt->second.v.data(), cin, cout, u, wc.get())) return answer(false, "fold_upsample");
        dump(out.f, "wc", {u * cout, cin, 3}, std::vector<float>(wc.get(), wc.get() + (size_t)u * cout * cin * 3));
        dump(out.f, "rows", {u * cout}, ck::row_bias(b->second, u));
        return answer(true);
    } else {
        return 2;
    }
    dump(out.f, a);
    return answer(true);
}
