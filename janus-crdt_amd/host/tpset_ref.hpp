// host/tpset_ref.hpp — TEST INFRASTRUCTURE ONLY: a dictionary-faithful C++ restatement of TPSet<string?>
// (MergeSharp/MergeSharp/CRDTs/2P-Set.cs), of TPSetMsg.Encode / Decode (:40-52) and of KeySpaceManager's
// CreateNewKVPair / OnNext (BFT-CRDT/CRDTManagers/KeySpaceManager.cs:121-178): the CPU counterpart of csrc/tpset.hip
// (with tpset_encode.hip) and csrc/keyspace.hip, the one-thread baseline of host/bench_keyspace.cpp and the checker
// of host/kat_keyspace.cpp.
// A HashSet that nothing is removed from enumerates in first-insertion order: a vector plus an index stands for it.
// tests/tpset_ref.py is the same restatement in Python; tests/test_tpset.py holds the two to the same bytes.
#pragma once

#include <cstdint>
#include <optional>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "json.hpp"  // oracle::json::EscapeTo (JavaScriptEncoder.Default)

namespace janus::ref {

using Elem = std::optional<std::string>;  // nullopt = the C# null element

class OrderedSet {  // HashSet<string?> under Add / Contains / UnionWith only
  public:
    bool Add(const Elem& e) {
        if (Contains(e)) return false;
        if (e) index_.emplace(*e, items_.size());
        else has_null_ = true;
        items_.push_back(e);
        return true;
    }
    bool Contains(const Elem& e) const { return e ? index_.count(*e) != 0 : has_null_; }
    void UnionWith(const std::vector<Elem>& other) {
        for (const auto& e : other) Add(e);
    }
    size_t Count() const { return items_.size(); }
    const std::vector<Elem>& items() const { return items_; }

  private:
    std::vector<Elem> items_;
    std::unordered_map<std::string, size_t> index_;
    bool has_null_ = false;
};

class TPSet {
  public:
    void Add(const Elem& e) { add_.Add(e); }                                          // 2P-Set.cs:106-109
    bool Contains(const Elem& e) const { return add_.Contains(e) && !rem_.Contains(e); }  // :169-172
    bool Remove(const Elem& e) {                                                      // :117-126
        if (!Contains(e)) return false;
        rem_.Add(e);
        return true;
    }
    long Count() const { return (long)add_.Count() - (long)rem_.Count(); }  // :76-82
    std::vector<Elem> LookupAll() const {                                   // :133-136
        std::vector<Elem> out;
        for (const auto& e : add_.items())
            if (!rem_.Contains(e)) out.push_back(e);
        return out;
    }
    void Merge(const std::vector<Elem>& add, const std::vector<Elem>& rem) {  // :188-192
        add_.UnionWith(add);
        rem_.UnionWith(rem);
    }
    const OrderedSet& addSet() const { return add_; }
    const OrderedSet& removeSet() const { return rem_; }
    // GetLastSynchronizedUpdate().Encode() (:210-213, :49-52): System.Text.Json's compact form
    std::string Encode() const {
        std::string o = "{\"addSet\":[";
        EncodeArray(o, add_.items());
        o += "],\"removeSet\":[";
        EncodeArray(o, rem_.items());
        o += "]}";
        return o;
    }

  private:
    static void EncodeArray(std::string& o, const std::vector<Elem>& items) {
        bool first = true;
        for (const auto& e : items) {
            if (!first) o.push_back(',');
            first = false;
            if (!e) {
                o += "null";
            } else {
                o.push_back('"');
                oracle::json::EscapeTo(o, *e);
                o.push_back('"');
            }
        }
    }
    OrderedSet add_, rem_;
};

// TPSetMsg.Decode (:40-46) under the accept contract of oracle/json.hpp: members in any order, unknown members
// skipped, a repeated member's last occurrence, arrays of strings or nulls in array order (duplicates kept; the sets
// drop them).  A member missing or null comes back without a value; malformed JSON throws JsonException.
struct Decoded {
    std::optional<std::vector<Elem>> add, rem;
};
inline Decoded Decode(std::string_view msg) {
    oracle::json::Reader r(msg);
    Decoded d;
    r.expect('{');
    if (!r.peek('}')) {
        do {
            const std::string name = r.string();
            r.expect(':');
            auto* member = name == "addSet" ? &d.add : name == "removeSet" ? &d.rem : nullptr;
            if (!member) {
                r.skip_value(1);
            } else if (r.null_literal()) {
                member->reset();
            } else {
                std::vector<Elem> items;
                r.expect('[');
                if (!r.peek(']')) {
                    do {
                        if (r.peek('"')) items.emplace_back(r.string());
                        else if (r.null_literal()) items.emplace_back(std::nullopt);
                        else r.fail("not a string");
                    } while (r.eat(','));
                }
                r.expect(']');
                *member = std::move(items);
            }
        } while (r.eat(','));
    }
    r.expect('}');
    r.end();
    return d;
}

// ApplySynchronizedUpdate message after message, with the key-space set's rule for a missing removeSet: 0 = merged,
// 1 = nothing applied (malformed, or addSet missing / null), 2 = addSet merged only (removeSet missing / null).
inline int MergeJson(TPSet& set, std::string_view msg) {
    Decoded d;
    try {
        d = Decode(msg);
    } catch (const oracle::json::JsonException&) {
        return 1;
    }
    if (!d.add) return 1;
    if (!d.rem) {
        set.Merge(*d.add, {});
        return 2;
    }
    set.Merge(*d.add, *d.rem);
    return 0;
}

// KeySpaceManager: the key-space CRDT, keySpaces (:30) and LastKeySpaceSet (:35).  Receive = the CRDT's
// ApplySynchronizedUpdate followed by OnNext (:151-178), in the reference's order: the null element first (it is
// dereferenced before any lookup), then ContainsKey of the bytes before the first NUL (the whole entry if it has none):
// an entry of a key the dictionary holds is skipped whatever the rest of it looks like.  Stated departure from the
// reference, which throws out of OnNext (and so wedges) there: an entry of an unknown key without a NUL (status 1) or
// with a guid segment not in "D" form (2), and the null element (3), is journalled with its raw bytes, not added, and
// processing goes on.  tests/tpset_ref.py KeySpaceRef is the same in Python.
class KeySpace {
  public:
    struct Record {
        std::string bytes;  // the key (status 0) or the raw entry
        oracle::Guid guid;
        int status;
    };
    bool CreateNewKVPair(const std::string& key, const oracle::Guid& guid) {  // :121-136
        const bool added = keys_.emplace(key, guid).second;                   // TryAdd
        set_.Add(key + std::string(1, '\0') + oracle::json::GuidD(guid));
        return added;
    }
    int Receive(std::string_view msg) {  // MergeJson's verdict; OnNext only after a whole merge
        const int st = MergeJson(set_, msg);
        if (st == 0) OnNext();
        return st;
    }
    void OnNext() {
        const std::vector<Elem> now = set_.LookupAll();
        for (const auto& e : now) {
            if (e ? last_.count(*e) != 0 : last_null_) continue;
            if (!e) {
                journal_.push_back({"", {}, 3});
                continue;
            }
            const size_t p1 = e->find('\0');
            const std::string key = e->substr(0, p1);
            if (keys_.count(key) != 0) continue;  // :164 ContainsKey first: Split(...)[1] and Guid.Parse never run
            if (p1 == std::string::npos) {
                journal_.push_back({*e, {}, 1});
                continue;
            }
            const size_t p2 = e->find('\0', p1 + 1);
            oracle::Guid g;
            if (!oracle::json::ParseGuidD(std::string_view(*e).substr(p1 + 1, p2 == std::string::npos ? std::string::npos : p2 - p1 - 1), g)) {
                journal_.push_back({*e, {}, 2});
                continue;
            }
            keys_.emplace(key, g);
            journal_.push_back({key, g, 0});
        }
        last_.clear();
        last_null_ = false;
        for (const auto& e : now) {
            if (e) last_.insert(*e);
            else last_null_ = true;
        }
    }
    const TPSet& set() const { return set_; }
    const std::unordered_map<std::string, oracle::Guid>& keys() const { return keys_; }
    const std::vector<Record>& journal() const { return journal_; }

  private:
    TPSet set_;
    std::unordered_map<std::string, oracle::Guid> keys_;
    std::unordered_set<std::string> last_;
    bool last_null_ = false;
    std::vector<Record> journal_;
};

}  // namespace janus::ref
