// Storage and entry points of the kernel-selection switches, generated from the table in tuning.h.  Host code only.
#include "dsg_common.h"
#include "tuning.h"

#include <cstdlib>
#include <cstring>

namespace dsg {
Tuning g_tune;
}

// Not part of the reference surface: a test / measurement hook; production processes keep the library's global state immutable.
DSG_API int dsg_set_tuning(int32_t key, int32_t value) {
  const char* t = getenv("DSG_TESTING");
  if (t == nullptr || t[0] != '1')
    return dsg::fail(DSG_ERR_INVALID_ARG, "dsg_set_tuning: kernel-selection switches are a test hook (set DSG_TESTING=1 in the "
                                          "environment); per-plan choices are in dsg_unet_config.flags");
  const int v = value;
  switch (key) {
#define DSG_TUNING_SET(k, field, dflt, ok) \
  case k:                                  \
    if (!(ok)) break;                      \
    dsg::g_tune.field = v;                 \
    ++dsg::g_tune.epoch;                   \
    return DSG_OK;
    DSG_TUNING_LIST(DSG_TUNING_SET)
#undef DSG_TUNING_SET
  }
  return dsg::fail(DSG_ERR_INVALID_ARG, "dsg_set_tuning: unknown key/value %d/%d", key, value);
}

DSG_API int32_t dsg_tuning_epoch(void) { return dsg::g_tune.epoch; }

DSG_API int dsg_get_tuning(int32_t key, int32_t* value) {
  DSG_CHECK_ARG(value != nullptr, "dsg_get_tuning: NULL pointer");
  switch (key) {
#define DSG_TUNING_GET(k, field, dflt, ok) \
  case k:                                  \
    *value = dsg::g_tune.field;            \
    return DSG_OK;
    DSG_TUNING_LIST(DSG_TUNING_GET)
#undef DSG_TUNING_GET
  }
  return dsg::fail(DSG_ERR_INVALID_ARG, "dsg_get_tuning: unknown key %d", key);
}

DSG_API int dsg_tuning_key(const char* name, int32_t* key) {
  DSG_CHECK_ARG(name != nullptr && key != nullptr, "dsg_tuning_key: NULL pointer");
#define DSG_TUNING_NAME(k, field, dflt, ok) \
  if (strcmp(name, #field) == 0) {          \
    *key = k;                               \
    return DSG_OK;                          \
  }
  DSG_TUNING_LIST(DSG_TUNING_NAME)
#undef DSG_TUNING_NAME
  return dsg::fail(DSG_ERR_INVALID_ARG, "dsg_tuning_key: no switch is called '%s'", name);
}
