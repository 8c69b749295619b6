// The navigation factors (GNSS, GnssFactor, ImuErrorFactor, ImuPosePriorFactor, ImuMixPriorFactor) are part of the product's host layer;
// the estimator port uses them in their default, 9-wide forms.
#pragma once
#include "../host/nav_factors.h"
