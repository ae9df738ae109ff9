// The header lane code of csrc/header_check.h on the CPU, as a stand-alone program (test-only):
// reads the rows tests/test_headers_host.py wrote from the model and the fixture, runs the lane
// functions the kernels run and compares.  Built plainly and with -fsanitize=address,undefined.
//
//   hash    <header hex> <hash hex>
//   expand  <bits> <target hex, 64 digits, most significant first> <flags>
//   compact <value hex> <bits>
//   pow     <hash hex> <bits> <limit hex> <0|1>
//   next    <last bits> <last time> <first time> <timespan> <limit hex> <no retargeting> <bits>
//   chain   <n> <limit hex> <timespan> <interval> <no retargeting> <bip34> <bip66> <bip65>
//           <max time> <height0> <genesis0> <prev bits> <prev hash hex> <period first time>
//           <n times> <times...> then n lines "<header hex> <status>"
// Hashes are raw digest bytes in hex; numbers are decimal.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "header_check.h"

using namespace bcc;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}
// a 64-digit number, most significant digit first, as limbs
static void limbs(const std::string& s, uint32_t (&out)[8]) {
    for (int j = 0; j < 8; j++) out[j] = (uint32_t)strtoul(s.substr(64 - 8 * (j + 1), 8).c_str(), nullptr, 16);
}
static void raw_limbs(const std::string& hex, uint32_t (&out)[8]) {
    const std::vector<uint8_t> b = unhex(hex);
    memcpy(out, b.data(), 32);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line, kind;
    size_t rows = 0, bad = 0;
    auto fail = [&](const std::string& what) {
        if (bad++ < 10) std::cerr << "mismatch: " << what << "\n";
    };
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        if (!(ss >> kind)) continue;
        rows++;
        if (kind == "hash") {
            std::string hdr, want;
            ss >> hdr >> want;
            // the header bytes at an odd address: the lane code reads them wherever they are
            std::vector<uint8_t> buf(1 + HEADER_BYTES);
            const std::vector<uint8_t> b = unhex(hdr);
            memcpy(buf.data() + 1, b.data(), HEADER_BYTES);
            uint32_t h[HEADER_WORDS], d[8], w[8];
            for (uint32_t k = 0; k < HEADER_WORDS; k++) h[k] = hdr_word(buf.data() + 1, k);
            header_hash_lane(h, d);
            raw_limbs(want, w);
            if (memcmp(d, w, 32) != 0) fail(line);
        } else if (kind == "expand") {
            uint32_t bits, flags, t[8], w[8];
            std::string target;
            ss >> bits >> target >> flags;
            limbs(target, w);
            if (compact_expand(bits, t) != flags || memcmp(t, w, 32) != 0) fail(line);
        } else if (kind == "compact") {
            std::string value;
            uint32_t bits, t[8];
            ss >> value >> bits;
            limbs(value, t);
            if (compact_get(t) != bits) fail(line);
        } else if (kind == "pow") {
            std::string hash, limit;
            uint32_t bits, d[8], l[8];
            int want;
            ss >> hash >> bits >> limit >> want;
            raw_limbs(hash, d);
            limbs(limit, l);
            if ((int)pow_check(d, bits, l) != want) fail(line);
        } else if (kind == "next") {
            HeaderRoundCtx c{};
            uint32_t last_bits, last_time, first_time, want;
            std::string limit;
            ss >> last_bits >> last_time >> first_time >> c.timespan >> limit >> c.no_retarget >> want;
            limbs(limit, c.pow_limit);
            if (next_work_required(last_bits, last_time, first_time, c) != want) fail(line);
        } else if (kind == "chain") {
            HeaderRoundCtx c{};
            size_t n;
            std::string limit, prev;
            ss >> n >> limit >> c.timespan >> c.interval >> c.no_retarget >> c.bip34 >> c.bip66 >> c.bip65 >>
                c.max_time >> c.height0 >> c.genesis0 >> c.prev_bits >> prev >> c.period_first_time >> c.n_times;
            limbs(limit, c.pow_limit);
            raw_limbs(prev, c.prev_hash);
            for (uint32_t k = 0; k < c.n_times && k < MTP_SPAN; k++) ss >> c.times[k];
            std::vector<uint8_t> hdr(1 + HEADER_BYTES * n), pow_ok(n);
            std::vector<uint32_t> hashes(8 * n);
            std::vector<int> want(n);
            for (size_t i = 0; i < n; i++) {
                std::string hx;
                std::getline(in, line);
                std::istringstream row(line);
                row >> hx >> want[i];
                const std::vector<uint8_t> b = unhex(hx);
                memcpy(hdr.data() + 1 + HEADER_BYTES * i, b.data(), HEADER_BYTES);
            }
            for (size_t i = 0; i < n; i++) {
                uint32_t h[HEADER_WORDS], d[8];
                for (uint32_t k = 0; k < HEADER_WORDS; k++) h[k] = hdr_word(hdr.data() + 1 + HEADER_BYTES * i, k);
                header_hash_lane(h, d);
                memcpy(&hashes[8 * i], d, 32);
                pow_ok[i] = pow_check(d, h[HW_BITS], c.pow_limit);
            }
            for (size_t i = 0; i < n; i++) {
                const int got = header_context_lane(hdr.data() + 1, hashes.data(), pow_ok.data(), (uint32_t)i, c);
                if (got != want[i]) fail("chain header " + std::to_string(i) + ": " + std::to_string(got) +
                                         " != " + std::to_string(want[i]));
            }
        } else {
            fail("unknown row " + kind);
        }
    }
    std::printf("%zu rows, %zu mismatches\n", rows, bad);
    return bad || !rows ? 1 : 0;
}
