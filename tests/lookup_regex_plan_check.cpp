// lookup_regex_plan_check.cpp — drives the plan arithmetic of bsg_match_rows_lookup_regex (bloomsearch_amd/csrc/host/lookup_plan.hpp
// with FieldRegex conditions, host/regex_groups.hpp build_blob_of) on the CPU for tests/test_match_lookup_regex_plan.py.  Input: a file
// of little-endian u64 words, [n_cases] then each case beginning with its kind; output: a file of u64 answers.  Plain C++: builds with
// g++ alone, and under -fsanitize=address,undefined as it stands.  A string is given as its length and one word per byte.
//   kind 0  table   n_conds, (kind, field string, token or pattern string)[n_conds], n_queries, (n_ops, op[n_ops])[n_queries],
//                   n_sets, set_query_off[n_sets + 1], set_queries[set_query_off[n_sets]]
//                   -> status and bad of build_strings as the plain lookup call makes it, then of the regex-tolerant form; Ok:
//                   n_strings, string_of[2 n_conds], canon[n_conds], n_pairs, n_rx, rx_conds[n_rx], rx_slot[n_conds], set_rx_masks[n_sets]
//   kind 1  cap     n_str_slots, n_pair_slots, n_strings, n_pairs -> lookup_lds_bytes, rx_lds_cap of the slots, rx_lds_cap_of the counts
//   kind 2  blob    cap, n_conds, (kind, field string, pattern string)[n_conds]
//                   -> build_strings status (regex form); Ok: blob status, the condition named, n_rx, the estimates [n_rx when every
//                   pattern compiled], blob bytes, per regex slot header word 1 >> 16 (the condition) and header word 2 >> 16 (field length)
//   kind 3  dfa     pattern string, field length -> compiled (0 / 1), n_states, n_classes, rx_table_bytes (single-call layout)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host/lookup_plan.hpp"
#include "host/regex_groups.hpp"

namespace {

struct In {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t take()
    {
        if (at >= w.size()) { fprintf(stderr, "case file ends early at word %zu\n", at); exit(2); }
        return w[at++];
    }
    std::string str()
    {
        std::string s((size_t)take(), '\0');
        for (char &c : s) c = (char)take();
        return s;
    }
};

struct Table {
    std::vector<uint32_t> kinds, off{0};
    std::string bytes;
    void read(In &in)
    {
        const uint32_t n = (uint32_t)in.take();
        for (uint32_t c = 0; c < n; ++c) {
            kinds.push_back((uint32_t)in.take());
            bytes += in.str();
            off.push_back((uint32_t)bytes.size());
            bytes += in.str();
            off.push_back((uint32_t)bytes.size());
        }
    }
    uint32_t n() const { return (uint32_t)kinds.size(); }
    const uint8_t *data() const { return (const uint8_t *)bytes.data(); }
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin answers.bin\n", argv[0]); return 2; }
    In in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { perror(argv[1]); return 2; }
        uint64_t v;
        while (fread(&v, 8, 1, f) == 1) in.w.push_back(v);
        fclose(f);
    }
    std::vector<uint64_t> out;
    const uint64_t n_cases = in.take();
    for (uint64_t k = 0; k < n_cases; ++k) {
        const uint64_t kind = in.take();
        if (kind == 0) {
            Table t;
            t.read(in);
            std::vector<uint32_t> ops, poff{0};
            const uint32_t nq = (uint32_t)in.take();
            for (uint32_t q = 0; q < nq; ++q) {
                const uint32_t n_ops = (uint32_t)in.take();
                for (uint32_t i = 0; i < n_ops; ++i) ops.push_back((uint32_t)in.take());
                poff.push_back((uint32_t)ops.size());
            }
            const uint32_t n_sets = (uint32_t)in.take();
            std::vector<uint32_t> sq_off(n_sets + 1), sq;
            for (auto &x : sq_off) x = (uint32_t)in.take();
            sq.resize(sq_off[n_sets]);
            for (auto &x : sq) x = (uint32_t)in.take();
            bsh_lookup::Plan plain, pl;
            uint32_t bad = 0;
            out.push_back((uint64_t)bsh_lookup::build_strings(t.data(), t.off.data(), t.kinds.data(), t.n(), plain, &bad));
            out.push_back(bad);
            bad = 0;
            const bsh_lookup::Status st = bsh_lookup::build_strings(t.data(), t.off.data(), t.kinds.data(), t.n(), pl, &bad, true);
            out.push_back((uint64_t)st);
            out.push_back(bad);
            if (st != bsh_lookup::Status::Ok) continue;
            out.push_back(pl.n_strings());
            out.insert(out.end(), pl.string_of.begin(), pl.string_of.end());
            out.insert(out.end(), pl.canon.begin(), pl.canon.end());
            out.push_back(pl.pairs.size());
            out.push_back(pl.rx_conds.size());
            out.insert(out.end(), pl.rx_conds.begin(), pl.rx_conds.end());
            for (uint32_t c = 0; c < t.n(); ++c) out.push_back(pl.rx_slot(c));
            const std::vector<uint32_t> masks = bsh_lookup::set_rx_masks(pl, ops.data(), poff.data(), nq, sq_off.data(), sq.data(), n_sets);
            out.insert(out.end(), masks.begin(), masks.end());
        } else if (kind == 1) {
            const uint32_t ss = (uint32_t)in.take(), ps = (uint32_t)in.take(), ns = (uint32_t)in.take(), np = (uint32_t)in.take();
            out.push_back(bsh_lookup::lookup_lds_bytes(ss, ps));
            out.push_back(bsh_lookup::rx_lds_cap(ss, ps));
            out.push_back(bsh_lookup::rx_lds_cap_of(ns, np));
        } else if (kind == 2) {
            const uint32_t cap = (uint32_t)in.take();
            Table t;
            t.read(in);
            bsh_lookup::Plan pl;
            const bsh_lookup::Status st = bsh_lookup::build_strings(t.data(), t.off.data(), t.kinds.data(), t.n(), pl, nullptr, true);
            out.push_back((uint64_t)st);
            if (st != bsh_lookup::Status::Ok) continue;
            std::vector<uint32_t> blob;
            const bsh_rxg::BlobResult r = bsh_rxg::build_blob_of(t.data(), t.off.data(), pl.rx_conds, cap, nullptr, blob);
            out.push_back((uint64_t)r.status);
            out.push_back(r.cond);
            out.push_back(r.n_rx);
            out.push_back(r.estimate.size());
            out.insert(out.end(), r.estimate.begin(), r.estimate.end());
            out.push_back(blob.size() * 4);
            if (r.status != bsh_rxg::BlobStatus::Ok) continue;
            for (uint32_t j = 0; j < r.n_rx; ++j) { out.push_back(blob[4 * j + 1] >> 16); out.push_back(blob[4 * j + 2] >> 16); }
        } else if (kind == 3) {
            const std::string pat = in.str();
            const uint32_t flen = (uint32_t)in.take();
            bsh_rx::Dfa d;
            std::string err;
            const bool ok = bsh_rx::compile(pat, d, err);
            out.push_back(ok);
            out.push_back(ok ? d.n_states : 0);
            out.push_back(ok ? d.n_classes : 0);
            out.push_back(ok ? bsh_rxg::rx_table_bytes(d.n_states, d.n_classes, flen, false) : 0);
        } else {
            fprintf(stderr, "unknown case kind %llu\n", (unsigned long long)kind);
            return 2;
        }
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (!out.empty() && fwrite(out.data(), 8, out.size(), f) != out.size()) { perror("write"); return 2; }
    fclose(f);
    return 0;
}
