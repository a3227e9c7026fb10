// device_pair.cpp — LikelihoodEngine::setDeviceRealignDiploid: the switch, and the one place of the adapter that names the C ABI's
// dd_compute_likelihoods_realign_diploid.  runBatch calls the entry through the pointer set here.
#include "compute_likelihoods.hpp"
#include "../../include/dindel_hmm.h"

namespace dindel {

void LikelihoodEngine::setDeviceRealignDiploid(bool v, int opsCap)
{
    deviceRealignDiploid_ = v;
    if (v) cigarOpsCap_ = opsCap < 1 ? 1 : opsCap;
    diploidEntry_ = reinterpret_cast<void (*)()>(&dd_compute_likelihoods_realign_diploid);
}

} // namespace dindel
