// The pose block's sizes: 7 parameters (position + quaternion), 6 local ones.  Part of factors.h; marginalization.h reads them.
#pragma once

#define POSE_LOCAL_SIZE 6
#define POSE_GLOBAL_SIZE 7
