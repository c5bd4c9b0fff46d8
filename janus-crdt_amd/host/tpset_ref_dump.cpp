// host/tpset_ref_dump.cpp — TEST ONLY: drives host/tpset_ref.hpp from a script on stdin so that tests/test_tpset.py
// can hold it to tests/tpset_ref.py byte for byte.  One command per line, strings as hex ("-" = the null element):
//   A <hex>   Add              prints nothing
//   R <hex>   Remove           prints 0 / 1
//   M <hex>   MergeJson of one encoded state   prints 0 merged / 1 nothing applied / 2 addSet only
//   C <hex> <lo> <hi>   KeySpace.CreateNewKVPair(key, guid) (decimal words)   prints 0 / 1
//   V <hex>   KeySpace.Receive of one encoded state (Merge + OnNext)   prints MergeJson's verdict
//   J         prints the key space's journal, one "status hex lo hi" line per record, then its set's wire bytes as
//             hex, then a fresh key space
//   E         Encode           prints the state's wire bytes as hex, the Count and LookupAll's size, then a fresh set
#include <cstdio>
#include <iostream>
#include <string>

#include "tpset_ref.hpp"

static janus::ref::Elem unhex(const std::string& h) {
    if (h == "-") return std::nullopt;
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

int main() {
    janus::ref::TPSet set;
    janus::ref::KeySpace ks;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        const std::string arg = line.size() > 2 ? line.substr(2) : "";
        if (line[0] == 'A') {
            set.Add(unhex(arg));
        } else if (line[0] == 'R') {
            std::printf("%d\n", set.Remove(unhex(arg)) ? 1 : 0);
        } else if (line[0] == 'M') {
            std::printf("%d\n", janus::ref::MergeJson(set, *unhex(arg)));
        } else if (line[0] == 'C') {
            const size_t a = arg.find(' '), b = arg.find(' ', a + 1);
            const oracle::Guid g{std::stoull(arg.substr(a + 1, b - a - 1)), std::stoull(arg.substr(b + 1))};
            std::printf("%d\n", ks.CreateNewKVPair(*unhex(arg.substr(0, a)), g) ? 1 : 0);
        } else if (line[0] == 'V') {
            std::printf("%d\n", ks.Receive(*unhex(arg)));
        } else if (line[0] == 'J') {
            for (const auto& r : ks.journal()) {
                std::printf("%d ", r.status);
                for (unsigned char c : r.bytes) std::printf("%02x", c);
                std::printf(" %llu %llu\n", (unsigned long long)r.guid.lo, (unsigned long long)r.guid.hi);
            }
            for (unsigned char c : ks.set().Encode()) std::printf("%02x", c);
            std::printf("\n");
            ks = janus::ref::KeySpace();
        } else if (line[0] == 'E') {
            for (unsigned char c : set.Encode()) std::printf("%02x", c);
            std::printf(" %ld %zu\n", set.Count(), set.LookupAll().size());
            set = janus::ref::TPSet();
        } else {
            return 2;
        }
    }
    return 0;
}
