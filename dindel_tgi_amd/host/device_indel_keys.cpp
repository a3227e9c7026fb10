// device_indel_keys.cpp — LikelihoodEngine::setDeviceIndelKeys: the switch, and the one place of the adapter that names the C ABI's
// dd_compute_likelihoods_faster_keys.  runBatch calls the entry through the pointer set here (as device_pair.cpp does for its entry: a
// program that stubs the C ABI without this entry and never sets the switch links).
#include "compute_likelihoods.hpp"
#include "../../include/dindel_hmm.h"

namespace dindel {

void LikelihoodEngine::setDeviceIndelKeys(bool v)
{
    deviceIndelKeys_ = v;
    indelKeysEntry_ = reinterpret_cast<void (*)()>(&dd_compute_likelihoods_faster_keys);
}

} // namespace dindel
