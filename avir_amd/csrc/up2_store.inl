// up2_store.inl -- k_up2< true, IO != 0 >'s stores of the caller's pixels,
// included by up2.hip inside the kernel's transposed vertical phase (they
// capture the lane's destination offsets dlv / dlv2, the row pitch, and for
// IO 8 / 9 the gamma parameters P.G).
		// IO != 0: a lane's two channels through the output stage (round
		// half up by truncation, clamp; the x86 build's cast beyond the int
		// range: plan.h) into the caller's image
		auto store_io = [&]( const f2 v, const __amdgpu_buffer_rsrc_t rs,
			const int soff )
		{
			if constexpr( IO == 7 )
			{
				// (a plain conversion of the pair, ONE v_cvt_pk_bf16_f32: nearest
				// even, float denormals become bfloat16 denormals, beyond the
				// largest finite one +-Inf)
				typedef __bf16 bf2 __attribute__(( ext_vector_type( 2 )));
				__builtin_amdgcn_raw_buffer_store_b32( __builtin_bit_cast(
					unsigned, __builtin_convertvector( v, bf2 )), rs, dlv, soff,
					U2_STAUX );
			}
			else
			if constexpr( IO == 6 )
			{
				// (plain conversions: v_cvt_f16_f32 rounds to nearest even and
				// keeps half denormals; the pkrtz form would truncate)
				const float v0 = v.x, v1 = v.y;
				const unsigned h0 = __builtin_bit_cast( unsigned short,
					(_Float16) v0 );
				const unsigned h1 = __builtin_bit_cast( unsigned short,
					(_Float16) v1 );
				__builtin_amdgcn_raw_buffer_store_b32( h0 | ( h1 << 16 ), rs, dlv,
					soff, U2_STAUX );
			}
			else
			if constexpr( IO == 3 )
			{
				// (element by element: __builtin_bit_cast of `v.y` stored v.x)
				const float v0 = v.x, v1 = v.y;
				__builtin_amdgcn_raw_buffer_store_b32( __float_as_uint( v0 ), rs,
					dlv, soff, U2_STAUX );
				__builtin_amdgcn_raw_buffer_store_b32( __float_as_uint( v1 ), rs,
					dlv2, soff, U2_STAUX );
			}
			else
			if constexpr( IO == 4 || IO == 5 )
			{
				// (float) (int) ( v + 0.5f ), clamped to [0, PK], cast: the same
				// number as the integer ( v + 0.5f ) truncates to, clamped --
				// for every |v| < 2^31, and an integer image's results are
				// within a few hundred of [0, PK]
				constexpr int PKI = ( IO == 4 ? 255 : 65535 );
				const int q0 = min( max( (int) ( v.x + 0.5f ), 0 ), PKI );
				const int q1 = min( max( (int) ( v.y + 0.5f ), 0 ), PKI );

				if constexpr( IO == 4 )
				{
					__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) q0, rs,
						dlv, soff, U2_STAUX );
					__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) q1, rs,
						dlv2, soff, U2_STAUX );
				}
				else
				{
					__builtin_amdgcn_raw_buffer_store_b16( (unsigned short) q0, rs,
						dlv, soff, U2_STAUX );
					__builtin_amdgcn_raw_buffer_store_b16( (unsigned short) q1, rs,
						dlv2, soff, U2_STAUX );
				}
			}
			else
			{
				constexpr float PK = ( IO == 1 ? 255.0f : 65535.0f );
				float t0 = (float) (int) ( v.x + 0.5f );
				float t1 = (float) (int) ( v.y + 0.5f );
				t0 = fminf( fmaxf( t0, 0.0f ), PK );
				t1 = fminf( fmaxf( t1, 0.0f ), PK );
				t0 = avirhip_x86_round_fix( v.x, t0, PK );
				t1 = avirhip_x86_round_fix( v.y, t1, PK );

				if constexpr( IO == 1 )
				{
					__builtin_amdgcn_raw_buffer_store_b8(
						(unsigned char) (unsigned) t0, rs, dlv, soff, U2_STAUX );
					__builtin_amdgcn_raw_buffer_store_b8(
						(unsigned char) (unsigned) t1, rs, dlv2, soff, U2_STAUX );
				}
				else
				{
					__builtin_amdgcn_raw_buffer_store_b16(
						(unsigned short) (unsigned) t0, rs, dlv, soff, U2_STAUX );
					__builtin_amdgcn_raw_buffer_store_b16(
						(unsigned short) (unsigned) t1, rs, dlv2, soff, U2_STAUX );
				}
			}
		};

		// IO 8 / 9: the lane's two channels of output rows y0 + 1 (`od`) and,
		// with `ESTC`, y0 + 2 (`ed`) through the de-linearising stage: each byte
		// the count of thresholds <= v, all values of the step level by level
		// so that a level's LDS reads are independent; byte stores as IO 1 / 4.
		// IO 9 has no direct branch: its source is a uint8 / uint16 image, so
		// every linearised sample lies in [0, 1] and every sum within the gain
		// of the four filters, the product of their taps' absolute sums, which
		// up2_run has checked to be below 16 (Up2Data::gain16) -- finite and
		// inside the range the thresholds were searched in.
		// (ESTC: std::true_type / std::false_type, as R0C and MODEC are passed --
		// the count of values is a constant of the instance)
		// U2_GTHR 256 (an experiment's build, `make thr1k`): the LDS copy holds
		// the colour half alone and an alpha channel takes the stage's direct
		// expression -- 1 KB less, a multiply, a round and a clamp more.
		auto store_gn = [&]( const f2 od, const f2 ed, const auto ESTC,
			const __amdgpu_buffer_rsrc_t rs1, const __amdgpu_buffer_rsrc_t rs2,
			const int soff )
		{
			if constexpr( GOUT )
			{
			constexpr bool EST = decltype( ESTC )::value;
			constexpr int N = ( EST ? 4 : 2 );
			const float* const thr = ds_table< U2_GTHR >();
			const int c0 = ( threadIdx.x & 1 ) * 2; // the lane's first channel
			const bool al[ 2 ] = { c0 == P.G.alpha_index,
				c0 + 1 == P.G.alpha_index };
			const float* const t[ 2 ] = {
				thr + ( U2_GTHR == 512 && al[ 0 ] ? 256 : 0 ),
				thr + ( U2_GTHR == 512 && al[ 1 ] ? 256 : 0 ) };
			const float v[ 4 ] = { od.x, od.y, ed.x, ed.y };
			int lo[ N ] = {};

#pragma unroll
			for( int s = 128; s >= 1; s >>= 1 )
			{
				float th[ N ];
#pragma unroll
				for( int k = 0; k < N; k++ )
				{
					th[ k ] = t[ k & 1 ][ lo[ k ] + s ];
				}

#pragma unroll
				for( int k = 0; k < N; k++ )
				{
					lo[ k ] += ( v[ k ] >= th[ k ] ? s : 0 );
				}
			}

			if constexpr( U2_GTHR == 256 )
			{
#pragma unroll
				for( int k = 0; k < N; k++ )
				{
					lo[ k ] = ( al[ k & 1 ] ? ds_direct_byte( v[ k ], true, P.G ) :
						lo[ k ]);
				}
			}

			if constexpr( IO == 8 )
			{
				// k_epilogue_gamma_thr's direct branch (+-Inf, NaN, HDR-sized
				// samples: nothing an image holds), behind ONE wave-wide test
				// per row pair and outside the accumulation chains: a loop over
				// the lane's such values
				unsigned far = 0u;
#pragma unroll
				for( int k = 0; k < N; k++ )
				{
					far |= ( !( fabsf( v[ k ]) <= 16.0f ) ? 1u << k : 0u );
				}

				if( __builtin_amdgcn_ballot_w64( far != 0u ) != 0 )
				{
#pragma nounroll
					while( far != 0u )
					{
						const int kf = __builtin_ctz( far );
						far &= far - 1u;
						float vf = v[ 0 ];
#pragma unroll
						for( int k = 1; k < N; k++ )
						{
							vf = ( kf == k ? v[ k ] : vf );
						}

						const int bt = ds_direct_byte( vf, al[ kf & 1 ], P.G );
#pragma unroll
						for( int k = 0; k < N; k++ )
						{
							lo[ k ] = ( kf == k ? bt : lo[ k ]);
						}
					}
				}
			}

			__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) lo[ 0 ], rs1,
				dlv, soff + drow_b, U2_STAUX );
			__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) lo[ 1 ], rs1,
				dlv2, soff + drow_b, U2_STAUX );

			if constexpr( EST )
			{
				__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) lo[ 2 ], rs2,
					dlv, soff + 2 * drow_b, U2_STAUX );
				__builtin_amdgcn_raw_buffer_store_b8( (unsigned char) lo[ 3 ], rs2,
					dlv2, soff + 2 * drow_b, U2_STAUX );
			}
			}
		};

		// (`est` is a constant of the unrolled row: one of the two is left)
		auto store_g = [&]( const f2 od, const f2 ed, const bool est,
			const __amdgpu_buffer_rsrc_t rs1, const __amdgpu_buffer_rsrc_t rs2,
			const int soff )
		{
			if( est ) store_gn( od, ed, std::true_type(), rs1, rs2, soff );
			else store_gn( od, ed, std::false_type(), rs1, rs2, soff );
		};
