// The library's last-error message (include/brever_hip.h): written through brv::fail (status.h) by every
// translation unit and read through brv_last_error().
#include "../../include/brever_hip.h"
#include "status.h"

BRV_DEFINE_STATUS(brv_version, brv_last_error)
