// host/keyspace.cpp — janus::GpuKeySpace over jg_keyspace_* (see keyspace.hpp).
#include "keyspace.hpp"

#include <stdexcept>

namespace janus {

namespace {
void check(int rc, const char* what) {
    if (rc == JG_OK) return;
    char buf[512];
    jg_last_error(buf, sizeof buf);
    throw std::runtime_error(std::string(what) + ": " + buf);
}
}  // namespace

GpuKeySpace::GpuKeySpace(jg_ctx* ctx, uint64_t cap_keys, uint64_t cap_bytes) {
    check(jg_keyspace_create(ctx, cap_keys, cap_bytes, &ks_), "jg_keyspace_create");
    check(jg_keyspace_set(ks_, &set_), "jg_keyspace_set");
}

GpuKeySpace::~GpuKeySpace() { (void)jg_keyspace_destroy(ks_); }

bool GpuKeySpace::CreateNewKVPair(const std::string& key, const jg_guid& guid) {
    const uint64_t off[2] = {0, key.size()};
    uint8_t added = 0;
    check(jg_keyspace_create_keys(ks_, 1, off, reinterpret_cast<const uint8_t*>(key.data()), &guid, &added), "jg_keyspace_create_keys");
    return added != 0;
}

long GpuKeySpace::Receive(const std::vector<std::string>& messages, const std::function<void(const std::string&, const jg_guid&)>& on_new_key) {
    std::vector<uint64_t> off{0};
    std::string bytes;
    for (const auto& m : messages) {
        bytes += m;
        off.push_back(bytes.size());
    }
    uint64_t bad = UINT64_MAX, n_new = 0;
    uint8_t partial = 0;
    const int rc = jg_keyspace_receive(ks_, messages.size(), off.data(), reinterpret_cast<const uint8_t*>(bytes.data()), 0, &bad, &partial, &n_new);
    if (rc != JG_OK && bad == UINT64_MAX) check(rc, "jg_keyspace_receive");
    uint64_t to = 0, nb = 0;
    check(jg_keyspace_new_keys(ks_, journal_at_, &to, &nb, nullptr, nullptr, nullptr, nullptr), "jg_keyspace_new_keys");
    const uint64_t n = to - journal_at_;
    if (n) {
        std::vector<uint64_t> joff(n + 1);
        std::string jbytes(nb ? nb : 1, '\0');
        std::vector<jg_guid> guid(n);
        std::vector<uint8_t> status(n);
        uint64_t cap = jbytes.size();
        check(jg_keyspace_new_keys(ks_, journal_at_, &to, &cap, joff.data(), reinterpret_cast<uint8_t*>(jbytes.data()), guid.data(), status.data()),
              "jg_keyspace_new_keys");
        for (uint64_t i = 0; i < n; ++i)
            if (status[i] == 0) on_new_key(jbytes.substr(joff[i], joff[i + 1] - joff[i]), guid[i]);
        journal_at_ = to;
    }
    return bad == UINT64_MAX ? -1 : (long)bad;
}

std::string GpuKeySpace::Encode() {
    uint64_t n = 0;
    check(jg_tpset_encode_json(set_, &n, nullptr, 0), "jg_tpset_encode_json");
    std::string out(n, '\0');
    check(jg_tpset_encode_json(set_, &n, reinterpret_cast<uint8_t*>(out.data()), n), "jg_tpset_encode_json");
    return out;
}

std::optional<jg_guid> GpuKeySpace::Lookup(const std::string& key) {
    const uint64_t off[2] = {0, key.size()};
    jg_guid g{};
    uint8_t found = 0;
    check(jg_keyspace_lookup(ks_, 1, off, reinterpret_cast<const uint8_t*>(key.data()), &g, &found), "jg_keyspace_lookup");
    if (!found) return std::nullopt;
    return g;
}

}  // namespace janus
