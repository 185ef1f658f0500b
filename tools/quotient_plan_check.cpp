// The quotient planner as a stand-alone host program, for runs under a sanitizer on a CPU (tools/README.md has the build line):
// reads constraint-system blobs (tools/quotient_plan_digest.py --dump DIR writes them), runs parse_cs and choose_quotient_plan on each
// under every knob setting of the Python tool and prints the same document: SHA-256 of the full summary (8 + 14 (E + 1) words) and of
// every class program.  Given DIR/<name>.bin in the order of DIR/order.json the output equals tests/golden/quotient_plans.json.
//     quotient_plan_check DIR/fixture_k6.bin DIR/fixture_wide_k6.bin ...
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../zkevm-circuits_amd/csrc/quotient_plan.hpp"

using namespace zk::qplan;

namespace {

std::string sha256_hex(const uint8_t* data, size_t len) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<uint8_t> m(data, data + len);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(((uint64_t)len * 8) >> (8 * i)));
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 | m[off + 4 * i + 3];
        for (int i = 16; i < 64; ++i) w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t s[8];
        for (int i = 0; i < 8; ++i) s[i] = h[i];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[i] + w[i];
            const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
            for (int j = 7; j > 0; --j) s[j] = s[j - 1];
            s[4] += t1;
            s[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i) h[i] += s[i];
    }
    char hex[65];
    for (int i = 0; i < 8; ++i) snprintf(hex + 8 * i, 9, "%08x", h[i]);
    return hex;
}
std::string sha256_words(const std::vector<uint32_t>& w) { return sha256_hex((const uint8_t*)w.data(), 4 * w.size()); }      // little-endian host, as numpy's tobytes()

struct Setting { const char* label; std::vector<std::pair<const char*, const char*>> env; };
const char* const KNOB_NAMES[] = {"ZK_QUOTIENT_SPLIT", "ZK_QUOTIENT_ADDSPLIT", "ZK_QUOTIENT_GROUP", "ZK_QUOTIENT_DAG", "ZK_QUOTIENT_COSTGATE", "ZK_QUOTIENT_MAC", "ZK_QUOTIENT_CHUNK", "ZK_LOOKUP_PLAIN"};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s BLOB.bin ...\n", argv[0]); return 2; }
    const std::vector<Setting> settings = {
        {"default", {}}, {"QUOTIENT_SPLIT=0", {{"ZK_QUOTIENT_SPLIT", "0"}}}, {"QUOTIENT_ADDSPLIT=0", {{"ZK_QUOTIENT_ADDSPLIT", "0"}}}, {"QUOTIENT_GROUP=0", {{"ZK_QUOTIENT_GROUP", "0"}}},
        {"QUOTIENT_DAG=0", {{"ZK_QUOTIENT_DAG", "0"}}}, {"QUOTIENT_COSTGATE=0", {{"ZK_QUOTIENT_COSTGATE", "0"}}}, {"QUOTIENT_MAC=0", {{"ZK_QUOTIENT_MAC", "0"}}}, {"QUOTIENT_MAC=1", {{"ZK_QUOTIENT_MAC", "1"}}},
        {"QUOTIENT_CHUNK=0", {{"ZK_QUOTIENT_CHUNK", "0"}}}, {"QUOTIENT_CHUNK=1", {{"ZK_QUOTIENT_CHUNK", "1"}}}, {"LOOKUP_PLAIN=1", {{"ZK_LOOKUP_PLAIN", "1"}}},
        {"QUOTIENT_DAG=0,QUOTIENT_GROUP=0", {{"ZK_QUOTIENT_DAG", "0"}, {"ZK_QUOTIENT_GROUP", "0"}}}};
    std::vector<std::pair<std::string, std::vector<uint8_t>>> blobs;
    for (int i = 1; i < argc; ++i) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
        std::string name = argv[i];
        name = name.substr(name.find_last_of('/') + 1);
        if (name.size() > 4 && name.substr(name.size() - 4) == ".bin") name.resize(name.size() - 4);
        blobs.push_back({name, std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>())});
    }
    printf("{\n");
    bool first = true;
    for (const Setting& st : settings) {
        for (const char* name : KNOB_NAMES) unsetenv(name);
        for (const auto& kv : st.env) setenv(kv.first, kv.second, 1);
        for (const auto& nb : blobs) {
            Reader r{nb.second.data(), nb.second.size()};
            ConstraintSystem cs;
            std::string err;
            std::shared_ptr<const QuotientPlan> qp;
            if (parse_cs(r, &cs, nb.second.size(), false, &err) || choose_quotient_plan(cs, QuotientKnobs::read(), &qp, &err)) { fprintf(stderr, "%s: %s\n", nb.first.c_str(), err.c_str()); return 1; }
            std::vector<uint32_t> summary(8 + 14 * (size_t)(qp->E + 1), 0u);
            if (write_plan_summary(*qp, summary.data(), summary.size(), 0xFFFFFFFFu, nullptr, 0, nullptr)) { fprintf(stderr, "%s: no summary\n", nb.first.c_str()); return 1; }
            printf("%s\"%s|%s\": {\"summary\": \"%s\", \"classes\": [", first ? "" : ",\n", st.label, nb.first.c_str(), sha256_words(summary).c_str());
            first = false;
            for (uint32_t e = 0; e <= qp->E; ++e) {
                std::vector<uint32_t> words;
                for (const Instr& in : qp->cls[e].prog) { words.push_back(in.op); words.push_back(in.a); words.push_back(in.b); }
                printf("%s\"%s\"", e ? ", " : "", sha256_words(words).c_str());
            }
            printf("]}");
        }
    }
    printf("\n}\n");
    return 0;
}
