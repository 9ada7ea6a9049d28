// What cull.hip takes from the frame-instance stage (instances.hip owns it): the resident pairs of the context's last ivx_fi_views call.
#pragma once
#include "ivx_internal.hpp"

// *d_pairs: ivx_cull_pair[n_views x *n], view-major (null when *n == 0). IVX_ERR_STATE when the context's last ivx_fi_views call had another
// n_views, or there was none (`who` names the caller).
int ivx_fi_resident_pairs(ivx_ctx* c, const char* who, size_t n_views, const ivx_cull_pair** d_pairs, uint32_t* n);
