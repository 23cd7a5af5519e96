// AntreaProxy flows / groups (service.hpp). Flow text is golden-exact against
// pkg/agent/openflow/client_test.go:1024-1330 (Test_client_InstallServiceGroup,
// Test_client_InstallEndpointFlows, Test_client_InstallServiceFlows), for both families: a family-6
// Endpoint is loaded into / matched in xxreg3, its flows are tcp6 / udp6 / sctp6 with zone 65510.
#include "service.hpp"

#include <array>
#include <cstdio>
#include <cstring>
#include <tuple>

#include "core.hpp"

namespace gpc {

namespace {

// fields.go register marks used by the Service path
constexpr uint32_t kRewriteMac = 1u << 9;          // reg0[9]   RewriteMACRegMark
constexpr uint32_t kSvcNoEp = 1u << 14;            // reg0[14]  SvcNoEpRegMark
constexpr uint32_t kEpStateMask = 0x7u << 16;      // reg4[16..18] ServiceEPStateField
constexpr uint32_t kEpToSelect = 0x1u << 16;
constexpr uint32_t kEpSelected = 0x2u << 16;
constexpr uint32_t kEpToLearn = 0x3u << 16;        // EpToLearnRegMark (session affinity)
constexpr uint32_t kMaxInstallId = (1u << 24) - 1, kMaxNodePortId = 255;  // core.hpp aff_key
constexpr uint32_t kToNodePort = 1u << 19;         // reg4[19]  ToNodePortAddressRegMark
constexpr uint32_t kToExternal = 1u << 21;         // reg4[21]  ToExternalAddressRegMark
constexpr uint32_t kVirtualNodePortDNAT = 0xa9fe00fcu;  // config.VirtualNodePortDNATIPv4 169.254.0.252
constexpr uint32_t kRemoteEndpoint = 1u << 26;     // reg4[26]  RemoteEndpointRegMark
constexpr uint32_t kFromLocal = 1u << 28;          // reg4[28]  FromLocalRegMark
constexpr uint32_t kEpUnionMask = 0x7ffffu;        // reg4[0..18] EpUnionField
// config.VirtualNodePortDNATIPv6 fc01::aabb:ccdd:eefe (node_config.go:84)
constexpr uint8_t kVirtualNodePortDNAT6[16] = {0xfc, 0x01, 0, 0, 0, 0, 0, 0, 0, 0, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0xfe};

uint8_t ip_proto(uint8_t p) {  // gpc_protocol -> IP protocol number
  switch (p) {
    case GPC_PROTO_TCP: return 6;
    case GPC_PROTO_UDP: return 17;
    case GPC_PROTO_SCTP: return 132;
  }
  return 0;
}

const char* proto_name(uint8_t p, uint8_t family) {  // binding.Protocol string (cache keys)
  switch (p) {
    case GPC_PROTO_TCP: return family == 6 ? "tcp6" : "tcp";
    case GPC_PROTO_UDP: return family == 6 ? "udp6" : "udp";
    case GPC_PROTO_SCTP: return family == 6 ? "sctp6" : "sctp";
  }
  return "?";
}

IPAddr to_ip(const uint8_t* b, uint8_t family) {
  IPAddr a;
  a.fam = family == 6 ? 6 : 4;
  std::memcpy(a.b, b, a.fam == 4 ? 4 : 16);
  return a;
}

Action set_reg(uint32_t r, uint32_t v, uint32_t m = 0xffffffffu) {
  Action a{ACT_SET_REG};
  a.a = r;
  a.b = v;
  a.c = m;
  a.has_mask = m != 0xffffffffu;
  return a;
}

void match_reg(Match& m, int r, uint32_t v, uint32_t mask) {  // several marks of one register merge
  if (m.reg_present & (1u << r)) {
    m.reg_v[r] |= v;
    m.reg_m[r] |= mask;
  } else {
    m.set_reg(r, v, mask);
  }
}

uint64_t half(const IPAddr& a, int h) {  // big-endian 64-bit half of an IPv6 address
  uint64_t v = 0;
  for (int i = 0; i < 8; i++) v = (v << 8) | a.b[8 * h + i];
  return v;
}

void words_of(const uint8_t* b, uint32_t* w) {  // four big-endian 32-bit words, most significant first
  for (int k = 0; k < 4; k++)
    w[k] = (uint32_t(b[4 * k]) << 24) | (uint32_t(b[4 * k + 1]) << 16) | (uint32_t(b[4 * k + 2]) << 8) | b[4 * k + 3];
}

void set_proto(Match& m, uint8_t proto, uint8_t family) {
  m.has_dl = true;
  m.dl_type = family == 6 ? kEthIPv6 : kEthIP;
  m.has_proto = proto != 0;
  m.nw_proto = proto;
}

}  // namespace

FeatureService::FeatureService(const gpc_config& cfg) : cfg_(cfg) {}

uint64_t FeatureService::cookie() const {  // cookie.Service category of the same round
  return cfg_.cookie ? ((cfg_.cookie & ~(0xffull << 40)) | (3ull << 40)) : 0;
}

// serviceEndpointGroup (pipeline.go:2553-2592)
int FeatureService::install_service_group(uint32_t gid, bool affinity, const gpc_endpoint* eps, size_t n) {
  Group g;
  g.id = gid;
  const uint8_t resubmit = affinity ? TB_SERVICE_LB : TB_ENDPOINT_DNAT;
  if (n == 0) {
    Bucket b;
    b.acts = {set_reg(0, kSvcNoEp, kSvcNoEp)};
    Action r{ACT_RESUBMIT};
    r.a = TB_ENDPOINT_DNAT;
    b.acts.push_back(r);
    g.buckets.push_back(b);
  }
  for (size_t i = 0; i < n; i++) {
    const gpc_endpoint& e = eps[i];
    if (!family_ok(e.family)) return -GPC_EINVAL;
    Bucket b;
    b.id = uint32_t(i);
    if (!e.is_local && e.has_node_name && !e.is_node_ip) b.acts.push_back(set_reg(4, kRemoteEndpoint, kRemoteEndpoint));
    if (e.family == 6) {  // EndpointIP6Field (pipeline.go:2582-2584)
      const IPAddr a = to_ip(e.ip, 6);
      Action x{ACT_SET_XXREG3};
      x.lv = half(a, 0);
      x.lm = half(a, 1);
      b.acts.push_back(x);
    } else {
      b.acts.push_back(set_reg(3, to_ip(e.ip, 4).v4()));
    }
    b.acts.push_back(set_reg(4, e.port, 0xffff));
    Action r{ACT_RESUBMIT};
    r.a = resubmit;
    b.acts.push_back(r);
    g.buckets.push_back(b);
  }
  groups_[gid] = g;
  generation_++;
  return GPC_OK;
}

int FeatureService::uninstall_service_group(uint32_t gid) {
  groups_.erase(gid);
  generation_++;
  return GPC_OK;
}

static std::string endpoint_key(const gpc_endpoint& e, uint8_t proto) {  // generateEndpointFlowCacheKey
  char buf[96];
  std::snprintf(buf, sizeof buf, "E%s%s%x", to_ip(e.ip, e.family).str().c_str(), proto_name(proto, e.family), e.port);
  return buf;
}

// InstallEndpointFlows (client.go:750-770): endpointDNATFlow (pipeline.go:2502-2528) per Endpoint,
// plus podHairpinSNATFlow (pipeline.go:3052-3064) for local Endpoints.
int FeatureService::install_endpoint_flows(uint8_t proto, uint8_t family, const gpc_endpoint* eps, size_t n) {
  if (!ip_proto(proto) || !family_ok(family)) return -GPC_EINVAL;
  std::map<std::string, std::vector<Flow>> add;
  for (size_t i = 0; i < n; i++) {
    const gpc_endpoint& e = eps[i];
    if (e.family != family) return -GPC_EINVAL;
    const IPAddr addr = to_ip(e.ip, family);
    const uint32_t ip = addr.v4();
    std::vector<Flow> fl;
    Flow f;
    f.table = TB_ENDPOINT_DNAT;
    f.priority = kPriorityNormal;
    f.cookie = cookie();
    set_proto(f.m, ip_proto(proto), family);
    f.m.set_reg(4, kEpSelected | e.port, kEpUnionMask);
    Action ct{family == 6 ? ACT_CT_DNAT6 : ACT_CT_DNAT};
    ct.a = dnat_next_table();
    if (family == 6) {
      f.m.has_xxreg3 = true;
      std::memcpy(f.m.xxreg3, addr.b, 16);
      ct.b = kCtZoneV6;
      ct.c = e.port;
      ct.lv = half(addr, 0);
      ct.lm = half(addr, 1);
    } else {
      f.m.set_reg(3, ip);
      ct.b = kCtZone;
      ct.c = ip;
      ct.lv = e.port;
    }
    f.acts = {ct};
    fl.push_back(f);
    if (e.is_local) {
      Flow h;
      h.table = TB_SNAT_MARK;
      h.priority = kPriorityLow;
      h.cookie = cookie();
      h.m.has_ct_state = true;
      h.m.ct_data = 0x21;  // +new+trk
      h.m.ct_mask = 0x21;
      set_proto(h.m, 0, family);
      h.m.nw_src.set = h.m.nw_dst.set = true;
      h.m.nw_src.addr = h.m.nw_dst.addr = addr;
      Action hp{ACT_CT_HAIRPIN};
      hp.a = TB_SNAT;
      hp.b = family == 6 ? kCtZoneV6 : kCtZone;
      h.acts = {hp};
      fl.push_back(h);
    }
    add[endpoint_key(e, proto)] = fl;
  }
  for (auto& kv : add) cached_[kv.first] = kv.second;
  generation_++;
  return GPC_OK;
}

int FeatureService::uninstall_endpoint_flows(uint8_t proto, uint8_t family, const gpc_endpoint* eps, size_t n) {
  if (!ip_proto(proto) || !family_ok(family)) return -GPC_EINVAL;
  for (size_t i = 0; i < n; i++) cached_.erase(endpoint_key(eps[i], proto));
  generation_++;
  return GPC_OK;
}

static std::string service_key(const IPAddr& ip, uint16_t port, uint8_t proto) {  // generateServicePortFlowCacheKey
  char buf[96];
  std::snprintf(buf, sizeof buf, "S%s%s%x", ip.str().c_str(), proto_name(proto, ip.fam), port);
  return buf;
}

// InstallServiceFlows (client.go:790-807) -> serviceLBFlows (pipeline.go:2373-2431).
int FeatureService::install_service_flows(const gpc_service_config& c) {
  if (!ip_proto(c.protocol) || !family_ok(c.family)) return -GPC_EINVAL;
  if (c.is_dsr || c.is_nested) return -GPC_EINVAL;  // DSR / multi-cluster flows: not modelled
  // the short-circuit flow matches FromLocalRegMark: only batches of a packet_source context can tell
  const bool short_circuit = c.is_external && c.traffic_policy_local;
  if (short_circuit && !cfg_.packet_source) return -GPC_EINVAL;
  // learn flows: Services of a context with an affinity table for their family
  if (c.affinity_timeout && !(c.family == 6 ? cfg_.session_affinity6 : cfg_.session_affinity)) return -GPC_EINVAL;
  if (c.affinity_timeout && next_install_ >= kMaxInstallId) return -GPC_ENOMEM;
  const IPAddr ip = to_ip(c.ip, c.family);
  const uint32_t gid = c.traffic_policy_local ? c.local_group_id : c.cluster_group_id;  // TrafficPolicyGroupID
  Flow f;
  f.table = TB_SERVICE_LB;
  f.priority = kPriorityNormal;
  f.cookie = cookie();
  set_proto(f.m, ip_proto(c.protocol), c.family);
  f.m.has_tp_dst = true;
  f.m.tp_dst = c.port;
  f.m.tp_dst_m = 0xffff;
  match_reg(f.m, 4, kEpToSelect, kEpStateMask);
  if (c.is_nodeport) {  // ToNodePortAddressRegMark instead of the Service IP (pipeline.go:2381-2387)
    match_reg(f.m, 4, kToNodePort, kToNodePort);
  } else {
    f.m.nw_dst.set = true;
    f.m.nw_dst.addr = ip;
  }
  f.acts.push_back(set_reg(0, kRewriteMac, kRewriteMac));
  f.acts.push_back(set_reg(4, c.affinity_timeout ? kEpToLearn : kEpSelected, kEpStateMask));
  if (c.is_external) f.acts.push_back(set_reg(4, kToExternal, kToExternal));
  if (cfg_.enable_antrea_policy) f.acts.push_back(set_reg(7, gid));
  Action g{ACT_GROUP};
  g.a = gid;
  f.acts.push_back(g);
  std::vector<Flow> flows;
  if (short_circuit) {  // pipeline.go:2417-2422: from a local Pod or the Node -> the Cluster group
    Flow sc = f;
    sc.priority = kPriorityHigh;
    match_reg(sc.m, 4, kFromLocal, kFromLocal);
    for (auto& a : sc.acts) {
      if (a.kind == ACT_SET_REG && a.a == 7) a.b = c.cluster_group_id;
      if (a.kind == ACT_GROUP) a.a = c.cluster_group_id;
    }
    flows.push_back(sc);
  }
  flows.push_back(f);
  if (c.affinity_timeout) {  // serviceLearnFlow (pipeline.go:2316-2371)
    Flow l;
    l.table = TB_SERVICE_LB;
    l.priority = kPriorityLow;
    l.cookie = cookie() | gid;  // RequestWithObjectID(category, TrafficPolicyGroupID)
    set_proto(l.m, ip_proto(c.protocol), c.family);
    l.m.has_tp_dst = true;
    l.m.tp_dst = c.port;
    l.m.tp_dst_m = 0xffff;
    match_reg(l.m, 4, kEpToLearn, kEpStateMask);
    if (c.is_nodeport) {
      match_reg(l.m, 4, kToNodePort, kToNodePort);
    } else {
      l.m.nw_dst.set = true;
      l.m.nw_dst.addr = ip;
    }
    Action learn{ACT_LEARN};
    learn.a = c.affinity_timeout;
    learn.b = ip_proto(c.protocol);
    learn.c = (c.is_external ? 1u : 0u) | (c.family == 6 ? 2u : 0u);
    learn.lv = l.cookie;
    learn.lm = ++next_install_;  // the install id of its learned flows
    Action nx{ACT_GOTO};
    nx.a = TB_ENDPOINT_DNAT;
    l.acts = {learn, set_reg(4, kEpSelected, kEpStateMask), nx};
    flows.push_back(l);
  }
  cached_[service_key(ip, c.port, c.protocol)] = flows;
  generation_++;
  return GPC_OK;
}

int FeatureService::uninstall_service_flows(const uint8_t* ip, uint8_t family, uint16_t port, uint8_t proto) {
  if (!ip_proto(proto) || !family_ok(family)) return -GPC_EINVAL;
  cached_.erase(service_key(to_ip(ip, family), port, proto));
  generation_++;
  return GPC_OK;
}

int FeatureService::install_pod(const uint8_t* ip, uint8_t family, uint32_t ofport) {
  if (!family_ok(family)) return -GPC_EINVAL;
  if (family == 6) pods6_[to_ip(ip, 6)] = ofport;
  else pods_[to_ip(ip, 4).v4()] = ofport;
  generation_++;
  return GPC_OK;
}

int FeatureService::set_node_port_addresses(const uint8_t* ips, uint8_t family, size_t n) {
  if (!family_ok(family)) return -GPC_EINVAL;
  // cache keys: "NP" + address for IPv4, "N6" + address for IPv6 (one set per family)
  const char* const prefix = family == 6 ? "N6" : "NP";
  std::vector<IPAddr> addrs;
  for (size_t i = 0; i < n; i++) {
    const IPAddr a = to_ip(ips + 16 * i, family);
    bool loopback = a.b[0] == 127;  // loopback: not NodePort traffic from a Pod
    if (family == 6) {
      loopback = a.b[15] == 1;
      for (int k = 0; k < 15; k++) loopback = loopback && a.b[k] == 0;
    }
    if (!loopback) addrs.push_back(a);
  }
  if (n) {  // the gateway's DNATed NodePort connections
    uint8_t v[16] = {0};
    if (family == 6) std::memcpy(v, kVirtualNodePortDNAT6, 16);
    else for (int k = 0; k < 4; k++) v[k] = uint8_t(kVirtualNodePortDNAT >> (24 - 8 * k));
    addrs.push_back(to_ip(v, family));
  }
  if (family == 6 && cfg_.session_affinity6) {  // the same for the IPv6 addresses, ids of their own
    size_t fresh = 0;
    for (const IPAddr& a : addrs) fresh += !np_ids6_.count(a);
    if (np_ids6_.size() + fresh > kMaxNodePortId) return -GPC_EINVAL;
    for (const IPAddr& a : addrs)
      if (!np_ids6_.count(a)) {
        const uint32_t id = uint32_t(np_ids6_.size()) + 1;
        np_ids6_[a] = id;
      }
  }
  if (family == 4 && cfg_.session_affinity) {  // ids of the addresses, as the learned flows of NodePort Services key them
    size_t fresh = 0;
    for (const IPAddr& a : addrs) fresh += !np_ids_.count(a.v4());
    if (np_ids_.size() + fresh > kMaxNodePortId) return -GPC_EINVAL;
    for (const IPAddr& a : addrs)
      if (!np_ids_.count(a.v4())) {
        const uint32_t id = uint32_t(np_ids_.size()) + 1;
        np_ids_[a.v4()] = id;
      }
  }
  for (auto it = cached_.begin(); it != cached_.end();)
    it = it->first.compare(0, 2, prefix) == 0 ? cached_.erase(it) : std::next(it);
  for (const IPAddr& a : addrs) {
    Flow f;
    f.table = TB_NODEPORT_MARK;
    f.priority = kPriorityNormal;
    f.cookie = cookie();
    set_proto(f.m, 0, family);
    f.m.nw_dst.set = true;
    f.m.nw_dst.addr = a;
    f.acts.push_back(set_reg(4, kToNodePort, kToNodePort));
    char key[40];
    int o = std::snprintf(key, sizeof key, "%s", prefix);
    if (family == 6) {
      for (int k = 0; k < 16; k++) o += std::snprintf(key + o, sizeof key - size_t(o), "%02x", a.b[k]);
    } else {
      std::snprintf(key + o, sizeof key - size_t(o), "%08x", a.v4());
    }
    cached_[key] = {f};
  }
  generation_++;
  return GPC_OK;
}

int FeatureService::uninstall_pod(const uint8_t* ip, uint8_t family) {
  if (!family_ok(family)) return -GPC_EINVAL;
  if (family == 6) pods6_.erase(to_ip(ip, 6));
  else pods_.erase(to_ip(ip, 4).v4());
  generation_++;
  return GPC_OK;
}

uint32_t FeatureService::affinity_dst(uint32_t install, uint32_t np_id) const {
  for (auto& kv : cached_)
    for (auto& f : kv.second) {
      if (f.acts.empty() || f.acts[0].kind != ACT_LEARN || f.acts[0].lm != install) continue;
      if (f.m.nw_dst.set) return f.m.nw_dst.addr.v4();
      for (auto& np : np_ids_)
        if (np.second == np_id) return np.first;
    }
  return 0;
}

bool FeatureService::affinity_dst6(uint32_t install, uint32_t np_id, uint8_t* out) const {
  for (auto& kv : cached_)
    for (auto& f : kv.second) {
      if (f.acts.empty() || f.acts[0].kind != ACT_LEARN || f.acts[0].lm != install || f.m.dl_type != kEthIPv6) continue;
      if (f.m.nw_dst.set) {
        std::memcpy(out, f.m.nw_dst.addr.b, 16);
        return true;
      }
      for (auto& np : np_ids6_)
        if (np.second == np_id) {
          std::memcpy(out, np.first.b, 16);
          return true;
        }
    }
  std::memset(out, 0, 16);
  return false;
}

std::string FeatureService::dump_flows() const {
  std::string s;
  for (auto& kv : cached_)
    for (auto& f : kv.second) s += f.str() + "\n";
  return s;
}

std::string FeatureService::dump_groups() const {
  std::string s;
  for (auto& kv : groups_) s += kv.second.str() + "\n";
  return s;
}

// --------------------------------------------------------------------------- device image
namespace {

struct SvcHash {  // 2-choice cuckoo table of (key, value), kSvcSlots slots per bucket
  uint32_t log2 = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  bool build(const std::vector<std::pair<uint64_t, uint32_t>>& kv) {
    constexpr uint32_t S = kSvcSlots;
    for (log2 = 1; double(S << log2) * 0.6 < double(kv.size() + 1); log2++) {
    }
    for (int attempt = 0; attempt < 8; attempt++, log2++) {
      const uint32_t nb = 1u << log2, mask = nb - 1;
      keys.assign(size_t(nb) * S, 0);
      vals.assign(size_t(nb) * S, 0);
      bool ok = true;
      for (auto& e : kv) {
        uint64_t k = e.first;
        uint32_t v = e.second;
        int kicks = 0;
        while (true) {
          bool placed = false;
          for (uint32_t b : {hash_b1(k, mask), hash_b2(k, mask)}) {
            for (uint32_t i = 0; i < S && !placed; i++)
              if (!keys[size_t(b) * S + i]) {
                keys[size_t(b) * S + i] = k;
                vals[size_t(b) * S + i] = v;
                placed = true;
              }
            if (placed) break;
          }
          if (placed) break;
          if (++kicks > 500) {
            ok = false;
            break;
          }
          const uint32_t b = (kicks & 1) ? hash_b2(k, mask) : hash_b1(k, mask);
          const uint32_t i = uint32_t(kicks) % S;
          std::swap(k, keys[size_t(b) * S + i]);
          std::swap(v, vals[size_t(b) * S + i]);
        }
        if (!ok) break;
      }
      if (ok) return true;
    }
    return false;
  }
};

}  // namespace

// A group is an IPv6 one when a bucket loads xxreg3; a group without Endpoints belongs to no family.
static bool group_is_v6(const Group& g) {
  for (auto& b : g.buckets)
    for (auto& a : b.acts)
      if (a.kind == ACT_SET_XXREG3) return true;
  return false;
}
static bool group_is_v4(const Group& g) {
  for (auto& b : g.buckets)
    for (auto& a : b.acts)
      if (a.kind == ACT_SET_REG && a.a == 3) return true;
  return false;
}

// Pairs every priority-210 ServiceLB flow (`short_circuit`, per Service key) with the priority-200 flow
// of its key in `svcs`: that Service gets sc / sc_gid. A short-circuit flow without its priority-200
// flow, or one whose loads (reg7, EpToLearn) differ from it, is a shape the data path does not implement.
template <class Svc, class Map, class KeyFn>
static int pair_short_circuit(std::vector<Svc>& svcs, Map& short_circuit, KeyFn key_of, std::string* err) {
  for (auto& s : svcs) {
    const auto it = short_circuit.find(key_of(s));
    if (it == short_circuit.end()) continue;
    if (it->second.reg7 != s.reg7 || it->second.aff != s.aff) {
      *err = "ServiceLB short-circuit flow whose loads differ from its priority-200 flow (group " + std::to_string(s.gid) + ")";
      return -GPC_EINVAL;
    }
    s.sc = true;
    s.sc_gid = it->second.gid;
    short_circuit.erase(it);
  }
  if (!short_circuit.empty()) {
    *err = "ServiceLB short-circuit flow without its priority-200 flow (group " + std::to_string(short_circuit.begin()->second.gid) + ")";
    return -GPC_EINVAL;
  }
  return GPC_OK;
}

bool FeatureService::has_state(uint8_t family) const {
  for (auto& kv : cached_)
    for (auto& f : kv.second)
      if ((f.m.dl_type == kEthIPv6) == (family == 6)) return true;
  bool bare = false;  // a group without Endpoints
  for (auto& kv : groups_) {
    if (family == 6 ? group_is_v6(kv.second) : group_is_v4(kv.second)) return true;
    bare |= !group_is_v6(kv.second) && !group_is_v4(kv.second);
  }
  // groups without Endpoints alone keep an (empty) IPv4 image, unless the state is all IPv6
  return family == 4 && bare && !has_state(6);
}

int FeatureService::build_image(std::vector<uint32_t>* blob, std::string* err) const {
  blob->clear();
  if (!has_state(4)) return GPC_OK;
  // EndpointDNAT flows: (proto, endpoint ip, port) -> DNAT exists
  std::map<std::tuple<uint8_t, uint32_t, uint16_t>, bool> dnat;
  struct Svc {
    uint64_t key;
    uint32_t gid;
    bool reg7;
    bool aff;  // the ServiceLB flow loads EpToLearnRegMark: its learn flow follows the group
    bool sc = false;      // a short-circuit flow (priority 210, FromLocalRegMark) exists beside it ...
    uint32_t sc_gid = 0;  // ... to this (Cluster) group
  };
  struct Learn {
    uint32_t timeout, install;
  };
  std::map<uint64_t, Learn> learn;  // serviceLearnFlow per Service key
  std::vector<Svc> svcs;
  std::map<uint64_t, Svc> short_circuit;  // the priority-210 flows per Service key
  std::vector<uint32_t> node_port_addrs;
  bool any_node_port = false;
  for (auto& kv : cached_)
    for (auto& f : kv.second) {
      if (f.m.dl_type == kEthIPv6) continue;  // build_image6
      if (f.table == TB_NODEPORT_MARK) {
        if (!f.m.nw_dst.set || f.m.nw_dst.plen >= 0) {
          *err = "unsupported NodePortMark flow: " + f.str();
          return -GPC_EINVAL;
        }
        node_port_addrs.push_back(f.m.nw_dst.addr.v4());
      } else if (f.table == TB_ENDPOINT_DNAT) {
        if (!(f.m.reg_present & (1u << 3)) || !(f.m.reg_present & (1u << 4)) || f.acts.empty() ||
            f.acts[0].kind != ACT_CT_DNAT) {
          *err = "unsupported EndpointDNAT flow: " + f.str();
          return -GPC_EINVAL;
        }
        dnat[{f.m.nw_proto, f.m.reg_v[3], uint16_t(f.m.reg_v[4] & 0xffffu)}] = true;
      } else if (f.table == TB_SERVICE_LB) {
        // a NodePort Service (ToNodePortAddressRegMark, no Service IP) is keyed by address 0
        const bool node_port = (f.m.reg_present & (1u << 4)) && (f.m.reg_m[4] & kToNodePort) && (f.m.reg_v[4] & kToNodePort);
        any_node_port |= node_port;
        Svc s{svc_key(f.m.nw_proto, node_port ? 0u : f.m.nw_dst.addr.v4(), f.m.tp_dst), 0, false, false};
        const bool from_local = (f.m.reg_present & (1u << 4)) && (f.m.reg_m[4] & kFromLocal) && (f.m.reg_v[4] & kFromLocal);
        if (!f.acts.empty() && f.acts[0].kind == ACT_LEARN) {  // learn(...), EpSelected, goto EndpointDNAT
          const Action& l = f.acts[0];
          if ((f.m.reg_v[4] & kEpStateMask) != kEpToLearn || node_port == f.m.nw_dst.set || !f.m.has_tp_dst ||
              f.m.tp_dst_m != 0xffff || !l.a || !l.lm || l.lm > kMaxInstallId || f.acts.back().kind != ACT_GOTO ||
              f.acts.back().a != TB_ENDPOINT_DNAT) {
            *err = "unsupported ServiceLB learn flow: " + f.str();
            return -GPC_EINVAL;
          }
          learn[s.key] = Learn{l.a, uint32_t(l.lm)};
          continue;
        }
        bool grp = false;
        for (auto& a : f.acts) {
          if (a.kind == ACT_GROUP) s.gid = a.a, grp = true;
          if (a.kind == ACT_SET_REG && a.a == 7) s.reg7 = true;
          if (a.kind == ACT_SET_REG && a.a == 4 && a.c == kEpStateMask) s.aff = a.b == kEpToLearn;
        }
        if (!grp || node_port == f.m.nw_dst.set || (f.m.nw_dst.set && f.m.nw_dst.plen >= 0) || !f.m.has_tp_dst ||
            f.m.tp_dst_m != 0xffff) {
          *err = "unsupported ServiceLB flow: " + f.str();
          return -GPC_EINVAL;
        }
        if (from_local) {  // the short-circuit flow of the priority-200 flow with the same key
          if (f.priority != kPriorityHigh || short_circuit.count(s.key)) {
            *err = "unsupported ServiceLB short-circuit flow: " + f.str();
            return -GPC_EINVAL;
          }
          short_circuit[s.key] = s;
          continue;
        }
        svcs.push_back(s);
      }
    }
  if (const int rc = pair_short_circuit(svcs, short_circuit, [](const Svc& x) { return x.key; }, err)) return rc;
  std::vector<uint32_t> svc_words, ep_words, aff_ids;
  uint32_t n_aff = 0, n_sc = 0;
  std::vector<std::pair<uint64_t, uint32_t>> kv;
  for (auto& s : svcs) {
    const auto lit = learn.find(s.key);
    if (s.aff && lit == learn.end()) {
      *err = "ServiceLB flow loads EpToLearnRegMark without a learn flow (group " + std::to_string(s.gid) + ")";
      return -GPC_EINVAL;
    }
    // a short-circuit Service: its Local group's record, then its Cluster group's directly behind
    for (uint32_t r = 0; r < (s.sc ? 2u : 1u); r++) {
      const uint32_t gid = r ? s.sc_gid : s.gid;
      uint32_t first = uint32_t(ep_words.size() / 4), n = 0;
      auto git = groups_.find(gid);
      if (git != groups_.end() && group_is_v6(git->second)) {
        *err = "IPv4 Service with an IPv6 Endpoint group: " + git->second.str();
        return -GPC_EINVAL;
      }
      if (git != groups_.end()) {
        for (auto& b : git->second.buckets) {
          uint32_t ip = 0, port = 0, flags = 0;
          bool noep = false, to_dnat = false, to_lb = false;
          for (auto& a : b.acts) {
            if (a.kind == ACT_SET_REG && a.a == 3) ip = a.b;
            if (a.kind == ACT_SET_REG && a.a == 4 && a.c == 0xffffu) port = a.b;
            if (a.kind == ACT_SET_REG && a.a == 4 && (a.b & kRemoteEndpoint)) flags |= GPC_LB_REMOTE;
            if (a.kind == ACT_SET_REG && a.a == 0 && (a.b & kSvcNoEp)) noep = true;
            if (a.kind == ACT_RESUBMIT) to_dnat = a.a == TB_ENDPOINT_DNAT, to_lb = a.a == TB_SERVICE_LB;
          }
          // a session-affinity bucket resubmits to ServiceLB, where the Service's learn flow takes the
          // packet on to EndpointDNAT: bucket -> learn flow -> EndpointDNAT
          if (!(to_dnat || (to_lb && s.aff)) || (to_lb && noep)) {
            *err = "unsupported group bucket (session affinity): " + git->second.str();
            return -GPC_EINVAL;
          }
          if (s.aff && to_dnat && !noep) {
            *err = "session-affinity Service whose group bypasses its learn flow: " + git->second.str();
            return -GPC_EINVAL;
          }
          if (noep) continue;
          auto d = dnat.find({uint8_t((s.key >> 48) & 0xff), ip, uint16_t(port)});
          if (d != dnat.end()) flags |= GPC_LB_DNAT;
          uint32_t out_port = 0, dest = GPC_DEST_GATEWAY;
          auto pit = pods_.find(ip);
          if (pit != pods_.end()) {
            out_port = pit->second;
            dest = GPC_DEST_POD;
          } else if (flags & GPC_LB_REMOTE) {
            dest = GPC_DEST_TUNNEL;
          }
          ep_words.insert(ep_words.end(), {ip, port | (flags << 16), out_port, dest});
          n++;
        }
      }
      uint32_t lg = 6;
      while ((1u << lg) < n) lg++;
      if (n >= (1u << 24)) {
        *err = "too many Endpoints in one group";
        return -GPC_EINVAL;
      }
      if (r == 0) kv.push_back({s.key, uint32_t(svc_words.size() / 4)});
      svc_words.insert(svc_words.end(), {first, n | (lg << 24), gid,
                                         (s.reg7 ? kSvcLoadReg7 : 0u) | (s.aff ? kSvcAffinity | (lit->second.timeout << 16) : 0u) |
                                             (s.sc && r == 0 ? kSvcShortCircuit : 0u)});
      aff_ids.push_back(s.aff ? lit->second.install : 0u);
    }
    n_aff += s.aff;
    n_sc += s.sc;
  }
  SvcHash h;
  if (!h.build(kv)) {
    *err = "Service hash construction failed";
    return -GPC_ENOMEM;
  }
  const uint32_t nb = 1u << h.log2;
  SvcHdr hdr{};
  hdr.map_log2 = 12;  // about 16 map bits per Service: most non-Service packets stop at the map
  while (hdr.map_log2 < 22 && (1ull << hdr.map_log2) < 16ull * kv.size()) hdr.map_log2++;
  hdr.map_off = 32;
  hdr.hash_off = hdr.map_off + (1u << (hdr.map_log2 - 5));  // 128-B aligned
  hdr.hash_log2 = h.log2;
  hdr.svc_off = hdr.hash_off + nb * kSvcBucketWords;
  hdr.n_svc = uint32_t(svc_words.size() / 4);
  hdr.ep_off = hdr.svc_off + uint32_t(svc_words.size());
  hdr.n_ep = uint32_t(ep_words.size() / 4);
  // NodePort addresses: probed only when some ServiceLB flow is a NodePort one
  if (!any_node_port) node_port_addrs.clear();
  if (node_port_addrs.size() > kSvcMaxNodePortAddrs) {
    *err = "too many NodePort addresses";
    return -GPC_EINVAL;
  }
  hdr.np_off = hdr.ep_off + uint32_t(ep_words.size());
  hdr.n_np = uint32_t(node_port_addrs.size());
  // session affinity: the install id of every Service (0: none) and the id of every NodePort
  // address, after the rest -- an image without an affinity Service has neither
  hdr.n_aff = n_aff;
  hdr.n_sc = n_sc;
  hdr.aff_off = n_aff ? hdr.np_off + hdr.n_np : 0u;
  blob->assign(hdr.np_off + node_port_addrs.size() + (n_aff ? aff_ids.size() + node_port_addrs.size() : 0), 0u);
  std::copy(node_port_addrs.begin(), node_port_addrs.end(), blob->begin() + hdr.np_off);
  if (n_aff) {
    std::copy(aff_ids.begin(), aff_ids.end(), blob->begin() + hdr.aff_off);
    for (size_t i = 0; i < node_port_addrs.size(); i++) {
      const auto it = np_ids_.find(node_port_addrs[i]);
      (*blob)[hdr.aff_off + aff_ids.size() + i] = it == np_ids_.end() ? 0u : it->second;
    }
  }
  std::memcpy(blob->data(), &hdr, sizeof hdr);
  for (auto& e : kv) {
    const uint32_t mb = svc_map_bit(e.first, hdr.map_log2);
    (*blob)[hdr.map_off + (mb >> 5)] |= 1u << (mb & 31u);
  }
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t* w = blob->data() + hdr.hash_off + size_t(b) * kSvcBucketWords;
    for (uint32_t i = 0; i < kSvcSlots; i++) {
      const uint64_t k = h.keys[size_t(b) * kSvcSlots + i];
      w[kSvcSlotWords * i] = uint32_t(k);
      w[kSvcSlotWords * i + 1] = uint32_t(k >> 32);
      w[kSvcSlotWords * i + 2] = h.vals[size_t(b) * kSvcSlots + i];
    }
  }
  std::copy(svc_words.begin(), svc_words.end(), blob->begin() + hdr.svc_off);
  std::copy(ep_words.begin(), ep_words.end(), blob->begin() + hdr.ep_off);
  return GPC_OK;
}

int FeatureService::build_image6(std::vector<uint32_t>* blob, std::string* err) const {
  blob->clear();
  if (!has_state(6)) return GPC_OK;
  // EndpointDNAT flows: (proto, endpoint address, port) -> DNAT exists
  std::map<std::tuple<uint8_t, IPAddr, uint16_t>, bool> dnat;
  struct Svc {
    uint8_t proto;
    uint16_t port;
    uint32_t a[4];
    uint32_t gid;
    bool reg7;
    bool aff;  // the ServiceLB flow loads EpToLearnRegMark: its learn flow follows the group
    bool sc = false;      // a short-circuit flow (priority 210, FromLocalRegMark) exists beside it ...
    uint32_t sc_gid = 0;  // ... to this (Cluster) group
  };
  struct Learn {
    uint32_t timeout, install;
  };
  typedef std::tuple<uint8_t, uint16_t, std::array<uint32_t, 4>> SvcKey;  // (protocol, port, address; 0: NodePort)
  std::map<SvcKey, Learn> learn;  // serviceLearnFlow per Service key
  std::map<SvcKey, Svc> short_circuit;  // the priority-210 flows per Service key
  std::vector<Svc> svcs;
  std::vector<uint32_t> rec_svc;  // service record -> index into svcs
  std::vector<IPAddr> node_port_addrs;
  bool any_node_port = false;
  for (auto& kv : cached_)
    for (auto& f : kv.second) {
      if (f.m.dl_type != kEthIPv6) continue;
      if (f.table == TB_NODEPORT_MARK) {
        if (!f.m.nw_dst.set || f.m.nw_dst.plen >= 0) {
          *err = "unsupported NodePortMark flow: " + f.str();
          return -GPC_EINVAL;
        }
        node_port_addrs.push_back(f.m.nw_dst.addr);
      } else if (f.table == TB_ENDPOINT_DNAT) {
        if (!f.m.has_xxreg3 || !(f.m.reg_present & (1u << 4)) || f.acts.empty() || f.acts[0].kind != ACT_CT_DNAT6) {
          *err = "unsupported EndpointDNAT flow: " + f.str();
          return -GPC_EINVAL;
        }
        dnat[{f.m.nw_proto, to_ip(f.m.xxreg3, 6), uint16_t(f.m.reg_v[4] & 0xffffu)}] = true;
      } else if (f.table == TB_SERVICE_LB) {
        // a NodePort Service (ToNodePortAddressRegMark, no Service IP) is keyed by address 0
        const bool node_port = (f.m.reg_present & (1u << 4)) && (f.m.reg_m[4] & kToNodePort) && (f.m.reg_v[4] & kToNodePort);
        any_node_port |= node_port;
        Svc s{f.m.nw_proto, f.m.tp_dst, {0, 0, 0, 0}, 0, false, false};
        if (!node_port && f.m.nw_dst.set) words_of(f.m.nw_dst.addr.b, s.a);
        const bool from_local = (f.m.reg_present & (1u << 4)) && (f.m.reg_m[4] & kFromLocal) && (f.m.reg_v[4] & kFromLocal);
        if (!f.acts.empty() && f.acts[0].kind == ACT_LEARN) {  // learn(...), EpSelected, goto EndpointDNAT
          const Action& l = f.acts[0];
          if ((f.m.reg_v[4] & kEpStateMask) != kEpToLearn || node_port == f.m.nw_dst.set || !f.m.has_tp_dst ||
              f.m.tp_dst_m != 0xffff || !l.a || !l.lm || l.lm > kMaxInstallId || !(l.c & 2u) || f.acts.back().kind != ACT_GOTO ||
              f.acts.back().a != TB_ENDPOINT_DNAT) {
            *err = "unsupported ServiceLB learn flow: " + f.str();
            return -GPC_EINVAL;
          }
          learn[SvcKey{s.proto, s.port, {s.a[0], s.a[1], s.a[2], s.a[3]}}] = Learn{l.a, uint32_t(l.lm)};
          continue;
        }
        bool grp = false;
        for (auto& a : f.acts) {
          if (a.kind == ACT_GROUP) s.gid = a.a, grp = true;
          if (a.kind == ACT_SET_REG && a.a == 7) s.reg7 = true;
          if (a.kind == ACT_SET_REG && a.a == 4 && a.c == kEpStateMask) s.aff = a.b == kEpToLearn;
        }
        if (!grp || node_port == f.m.nw_dst.set || (f.m.nw_dst.set && f.m.nw_dst.plen >= 0) || !f.m.has_tp_dst ||
            f.m.tp_dst_m != 0xffff) {
          *err = "unsupported ServiceLB flow: " + f.str();
          return -GPC_EINVAL;
        }
        if (from_local) {  // the short-circuit flow of the priority-200 flow with the same key (build_image)
          const SvcKey key{s.proto, s.port, {s.a[0], s.a[1], s.a[2], s.a[3]}};
          if (f.priority != kPriorityHigh || short_circuit.count(key)) {
            *err = "unsupported ServiceLB short-circuit flow: " + f.str();
            return -GPC_EINVAL;
          }
          short_circuit[key] = s;
          continue;
        }
        svcs.push_back(s);
      }
    }
  if (const int rc = pair_short_circuit(svcs, short_circuit, [](const Svc& x) { return SvcKey{x.proto, x.port, {x.a[0], x.a[1], x.a[2], x.a[3]}}; }, err))
    return rc;
  std::vector<uint32_t> svc_words, ep_words, aff_ids;
  uint32_t n_aff = 0, n_sc = 0;
  std::vector<std::pair<uint64_t, uint32_t>> kv;
  for (auto& s : svcs) {
    const auto lit = learn.find(SvcKey{s.proto, s.port, {s.a[0], s.a[1], s.a[2], s.a[3]}});
    if (s.aff && lit == learn.end()) {
      *err = "ServiceLB flow loads EpToLearnRegMark without a learn flow (group " + std::to_string(s.gid) + ")";
      return -GPC_EINVAL;
    }
    for (uint32_t r = 0; r < (s.sc ? 2u : 1u); r++) {  // build_image
      const uint32_t gid = r ? s.sc_gid : s.gid;
      uint32_t first = uint32_t(ep_words.size() / kSvc6EpWords), n = 0;
      auto git = groups_.find(gid);
      if (git != groups_.end() && group_is_v4(git->second)) {
        *err = "IPv6 Service with an IPv4 Endpoint group: " + git->second.str();
        return -GPC_EINVAL;
      }
      if (git != groups_.end()) {
        for (auto& b : git->second.buckets) {
          IPAddr ip;
          ip.fam = 6;
          uint32_t port = 0, flags = 0;
          bool noep = false, to_dnat = false, to_lb = false;
          for (auto& a : b.acts) {
            if (a.kind == ACT_SET_XXREG3)
              for (int k = 0; k < 8; k++) {
                ip.b[k] = uint8_t(a.lv >> (56 - 8 * k));
                ip.b[8 + k] = uint8_t(a.lm >> (56 - 8 * k));
              }
            if (a.kind == ACT_SET_REG && a.a == 4 && a.c == 0xffffu) port = a.b;
            if (a.kind == ACT_SET_REG && a.a == 4 && (a.b & kRemoteEndpoint)) flags |= GPC_LB_REMOTE;
            if (a.kind == ACT_SET_REG && a.a == 0 && (a.b & kSvcNoEp)) noep = true;
            if (a.kind == ACT_RESUBMIT) to_dnat = a.a == TB_ENDPOINT_DNAT, to_lb = a.a == TB_SERVICE_LB;
          }
          // a session-affinity bucket resubmits to ServiceLB, where the Service's learn flow takes the
          // packet on to EndpointDNAT (build_image)
          if (!(to_dnat || (to_lb && s.aff)) || (to_lb && noep)) {
            *err = "unsupported group bucket (session affinity): " + git->second.str();
            return -GPC_EINVAL;
          }
          if (s.aff && to_dnat && !noep) {
            *err = "session-affinity Service whose group bypasses its learn flow: " + git->second.str();
            return -GPC_EINVAL;
          }
          if (noep) continue;
          if (dnat.count({s.proto, ip, uint16_t(port)})) flags |= GPC_LB_DNAT;
          uint32_t out_port = 0, dest = GPC_DEST_GATEWAY;
          auto pit = pods6_.find(ip);
          if (pit != pods6_.end()) {
            out_port = pit->second;
            dest = GPC_DEST_POD;
          } else if (flags & GPC_LB_REMOTE) {
            dest = GPC_DEST_TUNNEL;
          }
          uint32_t w[4];
          words_of(ip.b, w);
          ep_words.insert(ep_words.end(), {w[0], w[1], w[2], w[3], port | (flags << 16), out_port, dest, 0u});
          n++;
        }
      }
      uint32_t lg = 6;
      while ((1u << lg) < n) lg++;
      if (n >= (1u << 24)) {
        *err = "too many Endpoints in one group";
        return -GPC_EINVAL;
      }
      if (r == 0) kv.push_back({svc6_hash_key(s.proto, s.a, s.port), uint32_t(svc_words.size() / 4)});
      rec_svc.push_back(uint32_t(&s - svcs.data()));
      svc_words.insert(svc_words.end(), {first, n | (lg << 24), gid,
                                         (s.reg7 ? kSvcLoadReg7 : 0u) | (s.aff ? kSvcAffinity | (lit->second.timeout << 16) : 0u) |
                                             (s.sc && r == 0 ? kSvcShortCircuit : 0u)});
      aff_ids.push_back(s.aff ? lit->second.install : 0u);
    }
    n_aff += s.aff;
    n_sc += s.sc;
  }
  SvcHash h;
  if (!h.build(kv)) {
    *err = "Service hash construction failed";
    return -GPC_ENOMEM;
  }
  const uint32_t nb = 1u << h.log2;
  SvcHdr hdr{};
  hdr.map_log2 = 12;
  while (hdr.map_log2 < 22 && (1ull << hdr.map_log2) < 16ull * kv.size()) hdr.map_log2++;
  hdr.map_off = 32;
  hdr.hash_off = hdr.map_off + (1u << (hdr.map_log2 - 5));
  hdr.hash_log2 = h.log2;
  hdr.svc_off = hdr.hash_off + nb * kSvc6BucketWords;
  hdr.n_svc = uint32_t(svc_words.size() / 4);
  hdr.ep_off = hdr.svc_off + uint32_t(svc_words.size());
  hdr.n_ep = uint32_t(ep_words.size() / kSvc6EpWords);
  if (!any_node_port) node_port_addrs.clear();
  if (node_port_addrs.size() > kSvcMaxNodePortAddrs) {
    *err = "too many NodePort addresses";
    return -GPC_EINVAL;
  }
  hdr.np_off = hdr.ep_off + uint32_t(ep_words.size());
  hdr.n_np = uint32_t(node_port_addrs.size());
  // session affinity: the install id of every Service (0: none) and the id of every NodePort
  // address, after the rest -- an image without an affinity Service has neither
  hdr.n_aff = n_aff;
  hdr.n_sc = n_sc;
  hdr.aff_off = n_aff ? hdr.np_off + 4 * hdr.n_np : 0u;
  blob->assign(hdr.np_off + 4 * node_port_addrs.size() + (n_aff ? aff_ids.size() + node_port_addrs.size() : 0), 0u);
  for (size_t i = 0; i < node_port_addrs.size(); i++) words_of(node_port_addrs[i].b, blob->data() + hdr.np_off + 4 * i);
  if (n_aff) {
    std::copy(aff_ids.begin(), aff_ids.end(), blob->begin() + hdr.aff_off);
    for (size_t i = 0; i < node_port_addrs.size(); i++) {
      const auto it = np_ids6_.find(node_port_addrs[i]);
      (*blob)[hdr.aff_off + aff_ids.size() + i] = it == np_ids6_.end() ? 0u : it->second;
    }
  }
  std::memcpy(blob->data(), &hdr, sizeof hdr);
  for (auto& e : kv) {
    const uint32_t mb = svc_map_bit(e.first, hdr.map_log2);
    (*blob)[hdr.map_off + (mb >> 5)] |= 1u << (mb & 31u);
  }
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t* w = blob->data() + hdr.hash_off + size_t(b) * kSvc6BucketWords;
    for (uint32_t i = 0; i < kSvcSlots; i++) {
      if (!h.keys[size_t(b) * kSvcSlots + i]) continue;  // an empty slot: tag word 0 never matches
      const uint32_t si = h.vals[size_t(b) * kSvcSlots + i];
      const Svc& s = svcs[rec_svc[si]];
      uint32_t* slot = w + kSvc6SlotWords * i;
      for (int k = 0; k < 4; k++) slot[k] = s.a[k];
      slot[4] = svc6_tag(s.proto, s.port);
      slot[5] = si;
    }
  }
  std::copy(svc_words.begin(), svc_words.end(), blob->begin() + hdr.svc_off);
  std::copy(ep_words.begin(), ep_words.end(), blob->begin() + hdr.ep_off);
  return GPC_OK;
}

}  // namespace gpc
