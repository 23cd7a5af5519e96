// TEST-ONLY host run of the packet-in collection: core.hpp pin_records, the function the device
// passes evaluate, over a batch's verdict pairs and a packet-in image (gpc_debug_pin_image), serially
// in packet order -- the order the device's compaction must reproduce.
#include <cstring>

#include "core.hpp"

using namespace gpc;

extern "C" {

// verdicts: n pairs of gpc_verdict (16 B each); img: the packet-in image or null. Writes the first
// min(total, cap) records to recs and returns the total.
unsigned long long emu_pin_collect(const uint32_t* img, const uint32_t* verdicts, size_t n, gpc_packet_in* recs, size_t cap) {
  static_assert(sizeof(gpc_packet_in) == sizeof(PinRec), "a record is four words");
  unsigned long long total = 0;
  for (size_t i = 0; i < n; i++) {
    PinRec r[2];
    const uint32_t m = pin_records(uint32_t(i), verdicts + 4 * i, img, r);
    for (uint32_t s = 0; s < 2; s++) {
      if (!((m >> s) & 1u)) continue;
      if (total < cap) std::memcpy(&recs[total], &r[s], sizeof(PinRec));
      total++;
    }
  }
  return total;
}

// core.hpp pin_lookup of one id (0: not in the image).
uint32_t emu_pin_lookup(const uint32_t* img, uint32_t conj) { return pin_lookup(img, conj); }

// The image's keys: every non-empty {conj id, ops} slot of the hash, and whether each id's presence
// bit is set and pin_lookup finds it. Returns the number of slots written (cap pairs at most), or
// ~0 when a stored id fails its own lookup.
size_t emu_pin_entries(const uint32_t* img, uint32_t* pairs, size_t cap) {
  const PinHdr* h = reinterpret_cast<const PinHdr*>(img);
  size_t k = 0;
  for (size_t s = 0; s < (size_t(kPinSlots) << h->hash_log2); s++) {
    const uint32_t conj = img[h->hash_off + 2 * s], ops = img[h->hash_off + 2 * s + 1];
    if (!conj) continue;
    if (pin_lookup(img, conj) != ops) return ~size_t(0);
    if (k < cap) {
      pairs[2 * k] = conj;
      pairs[2 * k + 1] = ops;
    }
    k++;
  }
  return k;
}

uint32_t emu_pin_tile() { return kPinTile; }

}  // extern "C"
