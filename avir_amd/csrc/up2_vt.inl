// up2_vt.inl -- k_up2< true >'s vertical interpolation of ONE row, included by
// up2.hip inside the kernel's transposed vertical phase (it captures ea / oa,
// the 24 running sums). Row g of the ring (row rr of its marching step)
// carries c2 = C2[ m ]: the product fe[ t ] * c2 goes to even( m+3-t ), slot
// ( g + 3 - t ) % 12 of ea, and to odd( m-9+t ), slot ( g + 3 + t ) % 12 of oa.
// Which of the two sums want it is a compile-time matter of the step's MODE
// (up2_want_even / up2_want_odd, up2_chunks.h): a product is computed iff one
// of its sums is wanted, and a sum's +0 start is pruned with the sum. Every
// sum that is stored receives the same products in the same order in every
// mode, so the bits do not depend on it.
		auto vinterp = [&]( auto MODEC, const TapsE& V, const f2 c2,
			const int g, const int rr ) __attribute__(( always_inline ))
		{
			constexpr int MODE = decltype( MODEC )::value;

#pragma unroll
			for( int t = 0; t < 12; t += 2 )
			{
				const bool we0 = up2_want_even( MODE, g, rr, t );
				const bool wo0 = up2_want_odd( MODE, g, rr, t );
				const bool we1 = up2_want_even( MODE, g, rr, t + 1 );
				const bool wo1 = up2_want_odd( MODE, g, rr, t + 1 );
				f2 p0, p1;

				if( we0 || wo0 ) p0 = V.fe( t ) * c2;
				if( we1 || wo1 ) p1 = V.fe( t + 1 ) * c2;

				__builtin_amdgcn_sched_barrier( 0 );

				if( we0 )
				{
					f2& a = ea[ ( g + 3 - t + 24 ) % 12 ];
					a = ( t == 0 ? (f2) 0.0f : a ) + p0;
				}

				if( wo0 )
				{
					f2& a = oa[ ( g + 3 + t ) % 12 ];
					a = a + p0;
				}

				if( we1 )
				{
					f2& a = ea[ ( g + 2 - t + 24 ) % 12 ];
					a = a + p1;
				}

				if( wo1 )
				{
					f2& a = oa[ ( g + 4 + t ) % 12 ];
					a = ( t + 1 == 11 ? (f2) 0.0f : a ) + p1;
				}

				__builtin_amdgcn_sched_barrier( 0 );
			}

			// the pruned tail's pins (the other modes': after the call)
			if constexpr( MODE == 3 && U2_TAIL >= 2 )
			{
#pragma unroll
				for( int t = 0; t < 12; t++ )
				{
					if( up2_want_even( MODE, g, rr, t ))
					{
						asm volatile( "" : "+v"( ea[ ( g + 3 - t + 24 ) % 12 ]));
					}

					if( up2_want_odd( MODE, g, rr, t ))
					{
						asm volatile( "" : "+v"( oa[ ( g + 3 + t ) % 12 ]));
					}
				}
			}
		};
