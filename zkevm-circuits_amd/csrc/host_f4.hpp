// The host side's field element, 4 x u64 Montgomery limbs, alone (host_fq.hpp has the arithmetic): all that a header which only
// stores such values needs, so that it stays free of the device headers (cs.hpp, and through it quotient_lower.hpp).
#pragma once
#include <cstdint>

namespace zk {
namespace host {

struct F4 { uint64_t l[4]; };

}  // namespace host
}  // namespace zk
