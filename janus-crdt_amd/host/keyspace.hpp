// host/keyspace.hpp — C++ host mirror of KeySpaceManager (BFT-CRDT/CRDTManagers/KeySpaceManager.cs) over the C ABI
// (jg_keyspace_*, include/janus_gpu.h): what the C# layer of INTEGRATION.md §4 does, for the parity tests.
#pragma once

#include <functional>
#include <optional>
#include <string>
#include <vector>

#include "janus_gpu.h"

namespace janus {

class GpuKeySpace {
  public:
    GpuKeySpace(jg_ctx* ctx, uint64_t cap_keys, uint64_t cap_bytes);
    ~GpuKeySpace();
    GpuKeySpace(const GpuKeySpace&) = delete;
    GpuKeySpace& operator=(const GpuKeySpace&) = delete;

    // CreateNewKVPair (:121-136): false when the key was there already (the entry is added to the set regardless)
    bool CreateNewKVPair(const std::string& key, const jg_guid& guid);
    // The key-space CRDT's ApplySynchronizedUpdate + OnNext (:151-178) for each encoded state; on_new_key gets
    // (key, guid) per journalled key in order — the caller supplies the CRDT type and calls
    // GpuStableStore::CreateSafeCRDT (the reference takes the type from the replication manager,
    // SafeCRDTManager.cs:88).  Returns -1, or the index of the message the engine rejected (the keys journalled
    // before it are still delivered).
    long Receive(const std::vector<std::string>& messages, const std::function<void(const std::string&, const jg_guid&)>& on_new_key);
    std::string Encode();                                   // GetLastSynchronizedUpdate().Encode() of the set
    std::optional<jg_guid> Lookup(const std::string& key);  // keySpaces[key]
    jg_tpset* set() const { return set_; }
    jg_keyspace* handle() const { return ks_; }  // for GpuStableStore::QueryKeys (jg_node_query_keys)

  private:
    jg_keyspace* ks_ = nullptr;
    jg_tpset* set_ = nullptr;
    uint64_t journal_at_ = 0;  // journal records already delivered
};

}  // namespace janus
