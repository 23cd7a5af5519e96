// AntreaProxy feature of the classifier: the ServiceLB / EndpointDNAT flows
// and Endpoint groups of pkg/agent/openflow (client.go:710-815, pipeline.go:2374-2592, 3052), kept
// as the realized flow / group state OVS would hold, and the device Service image built from it.
#pragma once

#include <map>
#include <string>
#include <vector>

#include "gpc.h"
#include "model.hpp"

namespace gpc {

class FeatureService {
 public:
  explicit FeatureService(const gpc_config& cfg);

  int install_service_group(uint32_t gid, bool affinity, const gpc_endpoint* eps, size_t n);
  int uninstall_service_group(uint32_t gid);
  int install_endpoint_flows(uint8_t proto, uint8_t family, const gpc_endpoint* eps, size_t n);
  int uninstall_endpoint_flows(uint8_t proto, uint8_t family, const gpc_endpoint* eps, size_t n);
  int install_service_flows(const gpc_service_config& c);
  int uninstall_service_flows(const uint8_t* ip, uint8_t family, uint16_t port, uint8_t proto);
  int install_pod(const uint8_t* ip, uint8_t family, uint32_t ofport);
  // NodePort addresses (NewClient's nodePortAddressesIPv4 with proxyAll): the NodePortMark flows
  // (pipeline.go:2282-2314) for each non-loopback address and the virtual NodePort DNAT IP. One set
  // per family (featureService.nodePortAddresses[ipProtocol]): a call replaces its family's flows.
  // `ips`: n addresses of 16 bytes each (an IPv4 address in the first 4)
  int set_node_port_addresses(const uint8_t* ips, uint8_t family, size_t n);
  int uninstall_pod(const uint8_t* ip, uint8_t family);

  std::string dump_flows() const;   // FlowModToString lines of the realized Service flows
  std::string dump_groups() const;  // Group::str lines
  bool empty() const { return cached_.empty() && groups_.empty(); }
  // Session affinity (gpc_config.session_affinity): the destination a learned flow of install id
  // `install` and NodePort address id `np_id` matches (NXM_OF_IP_DST); 0 when no longer realized.
  uint32_t affinity_dst(uint32_t install, uint32_t np_id) const;
  // The same for an IPv6 learn flow (gpc_config.session_affinity6; NXM_NX_IPV6_DST): 16 bytes into
  // out, false (and zeros) when no longer realized.
  bool affinity_dst6(uint32_t install, uint32_t np_id, uint8_t* out) const;
  uint64_t generation() const { return generation_; }

  // Device Service image (core.hpp "Service image"), IPv4. Returns -GPC_EINVAL with *err for a
  // realized flow shape the data path does not implement.
  // Empty blob: no IPv4 Service state.
  int build_image(std::vector<uint32_t>* blob, std::string* err) const;
  // The IPv6 Service image (core.hpp "IPv6 Service image") from the tcp6 / udp6 / sctp6 ServiceLB
  // flows, the xxreg3 groups, the IPv6 EndpointDNAT / NodePortMark flows and the IPv6 Pod map.
  // Empty blob: no IPv6 Service state.
  int build_image6(std::vector<uint32_t>* blob, std::string* err) const;

 private:
  uint64_t cookie() const;
  uint8_t dnat_next_table() const { return cfg_.enable_antrea_policy ? TB_AP_EGRESS : TB_EGRESS; }

  gpc_config cfg_;
  std::map<std::string, std::vector<Flow>> cached_;  // featureService.cachedFlows: cache key -> flows
  std::map<uint32_t, Group> groups_;                 // featureService.groupCache
  std::map<uint32_t, uint32_t> pods_;                // IPv4 Pod IP -> ofport
  std::map<IPAddr, uint32_t> pods6_;                 // IPv6 Pod IP -> ofport
  bool family_ok(uint8_t family) const { return family == 4 || (family == 6 && cfg_.ipv6_enabled); }
  bool has_state(uint8_t family) const;              // some flow or group of that family is realized
  uint64_t generation_ = 0;
  // Session affinity. Install ids: one per install_service_flows of an affinity config, carried by
  // its learn flow (Action::lm), 24 bits, never reused. NodePort address ids: one per IPv4 NodePort
  // address ever set, 8 bits, never reused (the learned flows' NXM_OF_IP_DST of a NodePort Service).
  uint32_t next_install_ = 0;
  std::map<uint32_t, uint32_t> np_ids_;
  std::map<IPAddr, uint32_t> np_ids6_;  // the same for the IPv6 NodePort addresses (session_affinity6)
};

}  // namespace gpc
